! test_tt_rosenblatt_sq_real -- rosenblatt_sq_real of the drop-in tt_lib, the way back of sample_sq_real: points are drawn with
! sample_sq_real from the square of the interpolant of test_tt_sample_sq_real's signed rank-3 train, then mapped back.  One line per
! run: tag, the largest |u' - min(u,1)| over the drawn modes, whether logq and val repeated bit for bit (T / F), and the number of
! points whose cell is neither the sampler's nor the next one; first all modes drawn (auto mode), then mode 2 held at 0.3 with a
! defensive term in exact mode.  Before it one line per point, tag fx / hx: the point's number, u'(:), x(:), 17 digits each.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=5, npts=40
 type(dtt) :: a,b,c
 integer :: cell(d,npts),cell2(d,npts),k,j,p,off
 double precision :: u(d,npts),x(d,npts),u2(d,npts),lq(npts),v(npts),lq2(npts),v2(npts),nodes(6,d),cond(d),nan,err
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
 do k=1,d; do j=1,c%n(k); nodes(j,k)=0.d0+(1.d0-0.d0)*dble(j-1)/dble(c%n(k)-1); end do; end do
 do p=1,npts
  do k=1,d
   u(k,p)=mod(0.6180339887498949d0*(p+7*k)+0.37d0*p*k,1.d0)
  end do
 end do
 write(*,'(a,6i3)') 'ranks ',c%r(0:d)
 call sample_sq_real(c,u,nodes,x,cell=cell,logq=lq,val=v)
 call rosenblatt_sq_real(c,x,nodes,u2,cell=cell2,logq=lq2,val=v2)
 err=0.d0; off=0
 do p=1,npts
  do k=1,d
   err=max(err,abs(u2(k,p)-min(u(k,p),1.d0)))
   if(cell2(k,p).ne.cell(k,p).and.cell2(k,p).ne.cell(k,p)+1)off=off+1
  end do
  write(*,'(a,i4,10es26.17)') 'fx ',p,u2(:,p),x(:,p)
 end do
 write(*,'(a,es12.4,2l2,i4)') 'free ',err,all(transfer(lq2,1_8,npts).eq.transfer(lq,1_8,npts)),all(transfer(v2,1_8,npts).eq.transfer(v,1_8,npts)),off
 nan=0.d0; nan=nan/nan
 cond=nan; cond(2)=0.3d0
 call sample_sq_real(c,u,nodes,x,cond=cond,gamma=0.5d0,mode=0,cell=cell,logq=lq,val=v)
 x(2,:)=nan                                     ! the coordinate of a held mode is not looked at
 call rosenblatt_sq_real(c,x,nodes,u2,cond=cond,gamma=0.5d0,mode=0,cell=cell2,logq=lq2,val=v2)
 err=0.d0; off=0
 do p=1,npts
  if(cell2(2,p).ne.0.or.u2(2,p).ne.0.d0)error stop 'a held mode with a cell or a uniform'
  do k=1,d
   if(k.eq.2)cycle
   err=max(err,abs(u2(k,p)-min(u(k,p),1.d0)))
   if(cell2(k,p).ne.cell(k,p).and.cell2(k,p).ne.cell(k,p)+1)off=off+1
  end do
  write(*,'(a,i4,10es26.17)') 'hx ',p,u2(:,p),x(:,p)
 end do
 write(*,'(a,es12.4,2l2,i4)') 'held ',err,all(transfer(lq2,1_8,npts).eq.transfer(lq,1_8,npts)),all(transfer(v2,1_8,npts).eq.transfer(v,1_8,npts)),off
 call dealloc(a); call dealloc(b); call dealloc(c)
 write(*,'(a)') 'done'
end program
