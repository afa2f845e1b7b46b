! test_tt_compose -- dtt_dmrgg_trains of the drop-in dmrgg_lib (TTX_FUN_TRAINS on the device): the cross approximation of x*x for
! a train x built on the host, next to the program's own tijk(x,ind)**2.  Case 'rank1': x has rank 1 and entries +-2**e, so every
! product and quotient of the sweep is exact and the elements agree digit for digit; case 'rank2': entries of any kind, x*x has
! rank 3.  Lines: 'ranks' case, r(0:d) of the result; 'elem' case p, element of the result, tijk(x,ind)**2 (30 per case).
program main
 use tt_lib
 use dmrgg_lib
 use ttx_c
 implicit none
 integer,parameter :: d=4, npts=30
 type(dtt) :: a,b,x,z,z2
 type(dtt) :: ops(2)
 integer :: ind(d,npts),k,j,p,q
 integer(kind=8) :: neval
 double precision :: vx(npts),vz(npts)
 a%l=1; a%m=d; a%n(1:d)=[5,4,6,3]; call ones(a)
 b=a
 do k=1,d
  do j=1,a%n(k)
   a%u(k)%p(1,j,1)=(-1.d0)**(j*k)*2.d0**(mod(3*j+k,5)-2)
   b%u(k)%p(1,j,1)=cos(0.7d0*j+k)
  end do
 end do
 do p=1,npts
  q=11*(p-1)
  do k=1,d; ind(k,p)=1+mod(q,a%n(k)); q=q/a%n(k); end do
 end do
 ops(1)=a; ops(2)=a
 call dtt_dmrgg_trains(z,ops,TTX_TOP_PRODUCT,accuracy=1.d-13,maxrank=4,pivoting=2,neval=neval)
 write(*,'(a,5i4)') 'ranks rank1',z%r(0:d)
 vx=tijk(a,ind); vz=tijk(z,ind)
 do p=1,npts; write(*,'(a,i4,2es26.17)') 'elem rank1',p,vz(p),vx(p)**2; end do
 do k=1,d; do j=1,a%n(k); a%u(k)%p(1,j,1)=1.d0+0.25d0*j-0.1d0*k; end do; end do
 x=a+b                                          ! rank 2
 call dealloc(ops(1)); call dealloc(ops(2))
 ops(1)=x; ops(2)=x
 call dtt_dmrgg_trains(z2,ops,TTX_TOP_PRODUCT,accuracy=1.d-13,maxrank=6,pivoting=2,neval=neval)
 write(*,'(a,5i4)') 'ranks rank2',z2%r(0:d)
 vx=tijk(x,ind); vz=tijk(z2,ind)
 do p=1,npts; write(*,'(a,i4,2es26.17)') 'elem rank2',p,vz(p),vx(p)**2; end do
 call dealloc(a); call dealloc(b); call dealloc(x); call dealloc(z); call dealloc(z2); call dealloc(ops(1)); call dealloc(ops(2))
 write(*,'(a)') 'done'
end program
