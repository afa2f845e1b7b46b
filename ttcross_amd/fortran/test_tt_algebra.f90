! test_tt_algebra -- axpby / hadamard of the drop-in tt_lib (ttx_lincomb, ttx_hadamard on the device) next to the host + and * of
! the same module and to the program's own arithmetic on tijk.  x has rank 3, y rank 2, d = 5, built on the host.  Lines:
! 'ranks' of each result; 'elem' p, element of the result, the same value formed here from tijk of the operands (40 per result);
! 'same' T / F: every core of axpby(alpha,x,beta,y) equals the host alpha*x + beta*y bit for bit.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=5, npts=40
 type(dtt) :: a,b,x,y,r,h,z,r2,h2
 integer :: ind(d,npts),k,j,p,q
 double precision :: vr(npts),vx(npts),vy(npts),alpha,beta
 a%l=1; a%m=d; a%n(1:d)=[4,5,3,6,4]; call ones(a)
 b=a
 do k=1,d
  do j=1,a%n(k)
   a%u(k)%p(1,j,1)=1.d0+0.25d0*j-0.1d0*k
   b%u(k)%p(1,j,1)=cos(0.7d0*j+k)
  end do
 end do
 y=a+b                                          ! rank 2
 do k=1,d; do j=1,a%n(k); a%u(k)%p(1,j,1)=sin(1.3d0*j*k)+0.2d0; end do; end do
 x=y+a                                          ! rank 3
 do k=1,d; do j=1,a%n(k); y%u(k)%p(:,j,:)=y%u(k)%p(:,j,:)*(1.d0+0.1d0*sin(2.1d0*j+k)); end do; end do
 do p=1,npts
  q=37*(p-1)                                    ! 40 different points of the 4 x 5 x 3 x 6 x 4 modes
  do k=1,d; ind(k,p)=1+mod(q,x%n(k)); q=q/x%n(k); end do
 end do
 vx=tijk(x,ind); vy=tijk(y,ind)
 alpha=1.75d0; beta=-0.3d0
 r=axpby(alpha,x,beta,y)                        ! r takes the device train over
 h=(alpha*x)+(beta*y)
 write(*,'(a,6i4)') 'ranks axpby r',r%r(0:d)
 write(*,'(a,l2)') 'same axpby',same(r,h)
 vr=tijk(r,ind)
 do p=1,npts; write(*,'(a,i4,2es26.17)') 'elem ',p,vr(p),alpha*vx(p)+beta*vy(p); end do
 r2=axpby(1.d0,r,-2.d0,x)                       ! a resident operand and a host operand
 h2=(1.d0*h)+((-2.d0)*x)
 write(*,'(a,6i4)') 'ranks axpby2 r',r2%r(0:d)
 write(*,'(a,l2)') 'same axpby2',same(r2,h2)
 vr=tijk(r2,ind)
 do p=1,npts; write(*,'(a,i4,2es26.17)') 'elem ',p,vr(p),(alpha-2.d0)*vx(p)+beta*vy(p); end do
 z=hadamard(x,y)
 write(*,'(a,6i4)') 'ranks hadamard r',z%r(0:d)
 vr=tijk(z,ind)
 do p=1,npts; write(*,'(a,i4,2es26.17)') 'elem ',p,vr(p),vx(p)*vy(p); end do
 call dealloc(a); call dealloc(b); call dealloc(x); call dealloc(y); call dealloc(r); call dealloc(h); call dealloc(z)
 call dealloc(r2); call dealloc(h2)
 write(*,'(a)') 'done'
contains
 logical function same(p1,p2)
  type(dtt),intent(in) :: p1,p2
  integer :: kk
  same=.false.
  if(p1%m.ne.p2%m)return
  if(any(p1%r(0:p1%m).ne.p2%r(0:p1%m)))return
  do kk=1,p1%m
   if(any(shape(p1%u(kk)%p).ne.shape(p2%u(kk)%p)))return
   if(any(transfer(p1%u(kk)%p,[1_8]).ne.transfer(p2%u(kk)%p,[1_8])))return
  end do
  same=.true.
 end function
end program
