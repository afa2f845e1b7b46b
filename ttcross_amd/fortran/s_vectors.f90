! s_vector_mod -- drop-in for the fork's lib/s_vectors.f90: the 2^(d-1) sign vectors of the COS-coefficient sum.
! Column k (k = 1 .. 2^(d-1)) has s(1) = +1 and s(j) = -1 exactly where bit j-2 of k-1 is set.
module s_vector_mod
 implicit none
 integer,allocatable :: s_vectors(:,:)
contains
 subroutine generate_s_vectors(n_dimensions)
  integer,intent(in) :: n_dimensions
  integer :: k,j
  ! as in the fork: a set allocated earlier is reused (and must have the right shape)
  if(.not.allocated(s_vectors))allocate(s_vectors(n_dimensions,2**(n_dimensions-1)))
  do k=1,2**(n_dimensions-1)
   s_vectors(1,k)=1
   do j=2,n_dimensions
    s_vectors(j,k)=merge(-1,1,btest(k-1,j-2))
   end do
  end do
 end subroutine
end module s_vector_mod
