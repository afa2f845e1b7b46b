! test_tt_sample_sq_real -- sample_sq_real of the drop-in tt_lib: real points drawn from the SQUARE of the interpolant of a SIGNED
! rank-3 train of grid values built on the host, on equidistant nodes of [0,1], next to basisval (kind 2, the definition's
! operation order) at the same points.  One line per sample: tag, sample, val, basisval, logq, x; then the same with mode 2 held
! at 0.3, between two nodes, with a defensive term in exact mode.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=5, npts=40
 type(dtt) :: a,b,c
 integer :: cell(d,npts),k,j,p
 double precision :: u(d,npts),x(d,npts),lq(npts),v(npts),bv(npts),nodes(6,d),cond(d),nan
 a%l=1; a%m=d; a%n(1:d)=[4,5,3,6,4]; call ones(a)
 b=a
 do k=1,d
  do j=1,a%n(k)
   a%u(k)%p(1,j,1)=0.25d0*j-0.1d0*k-0.4d0
   b%u(k)%p(1,j,1)=cos(0.7d0*j+k)
  end do
 end do
 c=a+b
 do k=1,d; do j=1,a%n(k); a%u(k)%p(1,j,1)=sin(1.3d0*j*k); end do; end do
 c=c+a                                          ! rank 3, entries of both signs
 nodes=0.d0
 do k=1,d; do j=1,c%n(k); nodes(j,k)=0.d0+(1.d0-0.d0)*dble(j-1)/dble(c%n(k)-1); end do; end do   ! the nodes of basisval(.., 2, 0, 1, ..)
 do p=1,npts
  do k=1,d
   u(k,p)=mod(0.6180339887498949d0*(p+7*k)+0.37d0*p*k,1.d0)
  end do
 end do
 write(*,'(a,6i3)') 'ranks ',c%r(0:d)
 call sample_sq_real(c,u,nodes,x,cell=cell,logq=lq,val=v)
 call basisval(c,x,2,0.d0,1.d0,bv,mode=0)
 do p=1,npts
  if(any(cell(:,p).lt.1))error stop 'a drawn mode without a cell'
  write(*,'(a,i4,8es26.17)') 'free ',p,v(p),bv(p),lq(p),x(:,p)
 end do
 nan=0.d0; nan=nan/nan
 cond=nan; cond(2)=0.3d0
 call sample_sq_real(c,u,nodes,x,cond=cond,gamma=0.5d0,mode=0,cell=cell,logq=lq,val=v)
 call basisval(c,x,2,0.d0,1.d0,bv,mode=0)
 do p=1,npts
  if(cell(2,p).ne.0)error stop 'a held mode with a cell'
  write(*,'(a,i4,8es26.17)') 'held ',p,v(p),bv(p),lq(p),x(:,p)
 end do
 call dealloc(a); call dealloc(b); call dealloc(c)
 write(*,'(a)') 'done'
end program
