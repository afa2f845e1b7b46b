! funcs -- drop-in for the fork's lib/funcs.f90: the characteristic function of a multivariate normal distribution,
!   phi(omega) = exp(i omega'mu - omega'Sigma omega / 2).
module funcs
 implicit none
 private
 public :: gaussian_chf_nd
contains
 complex*16 function gaussian_chf_nd(n,omega,mu,sigma) result(phi)
  integer,intent(in) :: n
  double precision,intent(in) :: omega(n),mu(n),sigma(n,n)
  double precision :: lin,quad
  lin=sum(omega*mu)
  quad=sum(matmul(sigma,omega)*omega)
  phi=exp(dcmplx(0.d0,1.d0)*lin-0.5d0*quad)
 end function
end module funcs
