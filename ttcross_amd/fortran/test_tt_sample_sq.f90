! test_tt_sample_sq -- sample_sq of the drop-in tt_lib: indices drawn from the square of a SIGNED rank-3 train built on the host,
! next to tijk of the same indices.  One line per sample: tag, sample, val, tijk, logq; then the same with mode 2 held at index 3
! and a defensive term, in the exact mode.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=5, npts=40
 type(dtt) :: a,b,c
 integer :: ind(d,npts),fixed(d),k,j,p
 double precision :: u(d,npts),lq(npts),v(npts),vl
 a%l=1; a%m=d; a%n(1:d)=[4,5,3,6,4]; call ones(a)
 b=a
 do k=1,d
  do j=1,a%n(k)
   a%u(k)%p(1,j,1)=0.25d0*j-0.1d0*k-0.3d0
   b%u(k)%p(1,j,1)=cos(0.7d0*j+k)
  end do
 end do
 c=a+b
 do k=1,d; do j=1,a%n(k); a%u(k)%p(1,j,1)=sin(1.3d0*j*k)+0.2d0; end do; end do
 c=c+a                                          ! rank 3, entries of both signs
 do p=1,npts
  do k=1,d
   u(k,p)=mod(0.6180339887498949d0*(p+7*k)+0.37d0*p*k,1.d0)
  end do
 end do
 write(*,'(a,6i3)') 'ranks ',c%r(0:d)
 call sample_sq(c,u,ind,logq=lq,val=v)
 do p=1,npts
  vl=tijk(c,ind(:,p))
  write(*,'(a,i4,3es26.17,5i3)') 'free ',p,v(p),vl,lq(p),ind(:,p)
 end do
 fixed=0; fixed(2)=3
 call sample_sq(c,u,ind,fixed=fixed,gamma=0.5d0,mode=0,logq=lq,val=v)
 do p=1,npts
  vl=tijk(c,ind(:,p))
  write(*,'(a,i4,3es26.17,5i3)') 'held ',p,v(p),vl,lq(p),ind(:,p)
 end do
 call dealloc(a); call dealloc(b); call dealloc(c)
 write(*,'(a)') 'done'
end program
