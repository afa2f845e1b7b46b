! Fixture generator (test infrastructure): the GENUINE reference's COS-coefficient integrand (calc_coefficient of
! coefficients_mod, with s_vector_mod / funcs / constants) at the parameters of the fork's test_crs_coscoeff driver.
!   ref_coscoeff values          reads "d npts" and npts rows of d indices from stdin, prints one value per row
!   ref_coscoeff sweep d n r piv runs dtt_dmrgg on calc_coefficient (acc = 500 eps) and prints its per-sweep log
program ref_coscoeff
 use coefficients_mod
 use s_vector_mod
 use tt_lib
 use dmrgg_lib
 use default_lib
 implicit none
 include 'mpif.h'
 type(dtt) :: tt
 character(len=16) :: mode
 integer :: d, n, r, piv, npts, p, i, j, info
 integer(kind=8) :: neval
 integer, allocatable :: ind(:), nn(:)
 double precision, allocatable :: mean(:), cov(:,:)
 double precision :: sig, corr, x0, rate, tm, acc

 call get_command_argument(1, mode)
 if (trim(mode) == 'values') then
  read(*,*) d, npts
 else
  call readarg(2, d, 6); call readarg(3, n, 65); call readarg(4, r, 20); call readarg(5, piv, 1)
 end if
 ! the driver's parameter block: sigma = 0.4, corr = 0.5, X_0 = log(100), rate = 0, T = 1
 sig = 0.4d0; corr = 0.5d0; x0 = log(100.0d0); rate = 0.d0; tm = 1.d0
 allocate(mean(d), cov(d,d), ind(d), nn(d))
 do i = 1, d
  mean(i) = x0 + (rate - 0.5d0 * sig**2) * tm
 end do
 do i = 1, d
  do j = 1, d
   if (i == j) then
    cov(i,j) = sig * sig * tm
   else
    cov(i,j) = sig * corr * sig * tm
   end if
  end do
 end do
 call generate_s_vectors(d)
 call init_coefficients(d, mean, cov, lower=0.525170185988090843d0, upper=8.52517018598809173d0)
 if (trim(mode) == 'values') then
  nn = 0
  do p = 1, npts
   read(*,*) ind
   write(*,'(es25.17e3)') calc_coefficient(d, ind, nn)
  end do
 else
  call mpi_init(info)
  acc = 500 * epsilon(1.d0)
  tt%l = 1; tt%m = d; tt%n = n; tt%r = 1
  call alloc(tt)
  call dtt_dmrgg(tt, calc_coefficient, maxrank=r, accuracy=acc, pivoting=piv, neval=neval)
  write(*,'(a,i12,a)') '...with', neval, ' evaluations completed'
  call mpi_finalize(info)
 end if
end program
