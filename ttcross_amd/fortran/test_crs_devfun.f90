! test_crs_devfun -- dtt_dmrgg with an ordinary Fortran `fun` that has a twin written for the device.
! f(x) = (x_1+..+x_D) / (1 + x_1^2+..+x_D^2) on [0,1]^D, Gauss-Legendre quadrature (the box set-up of test_crs_stdnorm / test_crs_mvn).
! Run as it is, `fun` is evaluated on the host (ttx_set_integrand_host) while the sweep runs on the GPU.  With
!    TTX_DEVICE_FUN=<rational.hsaco>:rational
! in the environment (examples/devfun/rational.hip compiled with hipcc --genco) the SAME binary evaluates on the device: the
! function uses only + * /, so both runs print the same sweep lines and the same integral.
! CLI: D N RANK PIV
program main
 use tt_lib
 use dmrgg_lib
 use time_lib
 use quad_lib
 use default_lib
 use ttx_c
 implicit none
 include 'mpif.h'
 double precision,parameter :: a=0.d0,b=1.d0
 double precision :: acc
 include 'test_crs_box.inc'
 acc=500*epsilon(1.d0)
 call dtt_dmrgg(tt,integrand,par,maxrank=r,accuracy=acc,pivoting=piv,neval=neval,quad=qq)
 t2=timef()
 if(me.eq.0)then
  if(ttx_fun_id(tt%ttx).eq.TTX_FUN_DEVICE)then
   write(*,'(a)') 'integrand on the device (TTX_DEVICE_FUN)'
  else
   write(*,'(a)') 'integrand on the host (callback)'
  end if
 end if
 write(*,'(a,i12,a,e12.4,a)') '...with',neval,' evaluations completed in ',t2-t1,' sec.'
 val=dtt_quad(tt,qq)
 write(*,'(a,e50.40)') 'computed value:',val
 write(*,'(a)') 'Good bye.'
 call dealloc(tt)
 call mpi_finalize(info)
end program

double precision function integrand(m,ind,n,par) result(f)
 implicit none
 integer,intent(in) :: m
 integer,intent(in) :: ind(m),n(m)
 double precision,intent(in) :: par(*)
 double precision :: s1,s2,x
 integer :: i
 s1=0.d0; s2=0.d0
 do i=1,m; x=par(ind(i)); s1=s1+x; s2=s2+x*x; end do
 f=s1/(1.d0+s2)
end function
