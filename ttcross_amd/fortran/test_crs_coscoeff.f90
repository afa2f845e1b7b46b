! test_crs_coscoeff -- the fork's COS-coefficient tensor (test_crs_coscoeff.f90): TT-cross of calc_coefficient for a correlated
! Gaussian, same CLI (D N RANK PIV) and parameter block, without the HDF5 output; prints the per-sweep log.  dtt_dmrgg recognises
! calc_coefficient and runs the device integrand TTX_FUN_COSCOEFF (TTX_INTEGRAND=host forces the host callback instead).
program main
 use coefficients_mod
 use tt_lib
 use dmrgg_lib
 use time_lib
 use default_lib
 use ttx_c
 implicit none
 include 'mpif.h'
 type(dtt) :: tt
 integer :: d,n,r,piv,i,j,info,me
 integer(kind=8) :: neval
 double precision :: acc,x0,sig,corr,rate,tm,t1,t2
 double precision,allocatable :: mean(:),cov(:,:)
 call readarg(1,d,6)
 call readarg(2,n,65)
 call readarg(3,r,20)
 call readarg(4,piv,1)
 call mpi_init(info)
 call mpi_comm_rank(MPI_COMM_WORLD,me,info)
 acc=500*epsilon(1.d0)
 x0=log(100.0d0); sig=0.4d0; corr=0.5d0; rate=0.d0; tm=1.d0
 allocate(mean(d),cov(d,d))
 do i=1,d
  mean(i)=x0+(rate-0.5d0*sig**2)*tm
  do j=1,d
   if(i.eq.j)then
    cov(i,j)=sig*sig*tm
   else
    cov(i,j)=sig*corr*sig*tm
   end if
  end do
 end do
 call generate_s_vectors(d)
 call init_coefficients(d,mean,cov,lower=0.525170185988090843d0,upper=8.52517018598809173d0)
 t1=timef()
 tt%l=1; tt%m=d; tt%n=n; tt%r=1
 call alloc(tt)
 call dtt_dmrgg(tt,calc_coefficient,maxrank=r,accuracy=acc,pivoting=piv,neval=neval)
 t2=timef()
 if(me.eq.0)write(*,'(a,i12,a,e12.4,a)') '...with',neval,' evaluations completed in ',t2-t1,' sec.'
 if(me.eq.0)write(*,'(a,i2)') 'integrand: fun_id',ttx_fun_id(tt%ttx)        ! 5: the device integrand, 4: the host callback
 call dealloc(tt)
 call mpi_finalize(info)
end program
