! test_contract -- contract / marginals of the drop-in tt_lib (ttx_contract, ttx_marginals on the device) next to the program's
! own loops over tijk.  A train of rank 3 built on the host, d = 6; modes 2, 4 and 5 are kept, the others (a leading, an interior and a trailing run) summed against weights
! of mixed sign.  Lines: 'ranks' of the contracted train; 'elem' p, contracted element, the same sum formed here (40 of them);
! 'marg' k, i, marginal of a small train (d = 4), the same sum formed here.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=6, npts=40, ds=4
 type(dtt) :: a,b,c,w,res,s,ws
 integer :: keep(d),ind(d),i2(3,npts),k,j,p,q,i1,i3,i4,i6,i
 double precision :: vb(npts),vl,marg(6,ds),acc
 a%l=1; a%m=d; a%n(1:d)=[4,5,3,6,4,5]; call ones(a)
 b=a; w=a
 do k=1,d
  do j=1,a%n(k)
   a%u(k)%p(1,j,1)=1.d0+0.25d0*j-0.1d0*k
   b%u(k)%p(1,j,1)=cos(0.7d0*j+k)
   w%u(k)%p(1,j,1)=sin(0.9d0*j+0.3d0*k)          ! mixed sign
  end do
 end do
 c=a+b
 do k=1,d; do j=1,a%n(k); a%u(k)%p(1,j,1)=sin(1.3d0*j*k)+0.2d0; end do; end do
 c=c+a                                          ! rank 3
 keep=[0,1,0,1,1,0]
 call contract(c,keep,res,w)
 write(*,'(a,i3,a,4i3,a,3i3)') 'ranks m',res%m,' r',res%r(0:3),' n',res%n(1:3)
 do p=1,npts
  q=3*(p-1)                                     ! 40 different points of the 5 x 6 x 4 kept modes
  i2(1,p)=1+mod(q,c%n(2)); i2(2,p)=1+mod(q/c%n(2),c%n(4)); i2(3,p)=1+q/(c%n(2)*c%n(4))
 end do
 vb=tijk(res,i2)
 do p=1,npts
  vl=0.d0
  do i1=1,c%n(1); do i3=1,c%n(3); do i6=1,c%n(6)
   ind=[i1,i2(1,p),i3,i2(2,p),i2(3,p),i6]
   vl=vl+w%u(1)%p(1,i1,1)*w%u(3)%p(1,i3,1)*w%u(6)%p(1,i6,1)*tijk(c,ind)
  end do; end do; end do
  write(*,'(a,i4,2es26.17)') 'elem ',p,vb(p),vl
 end do
 ! marginals of a small train
 s%l=1; s%m=ds; s%n(1:ds)=[3,6,2,4]; call ones(s)
 b=s; ws=s
 do k=1,ds
  do j=1,s%n(k)
   s%u(k)%p(1,j,1)=0.5d0+cos(1.1d0*j*k)
   b%u(k)%p(1,j,1)=sin(0.4d0*j-k)
   ws%u(k)%p(1,j,1)=cos(0.6d0*j+0.2d0*k)
  end do
 end do
 s=s+b                                          ! rank 2
 call marginals(s,marg,ws)
 do k=1,ds
  do i=1,s%n(k)
   acc=0.d0
   do i1=1,s%n(1); do i3=1,s%n(2); do i4=1,s%n(3); do i6=1,s%n(4)
    ind(1:ds)=[i1,i3,i4,i6]
    if(ind(k).ne.i)cycle
    vl=1.d0
    do j=1,ds; if(j.ne.k)vl=vl*ws%u(j)%p(1,ind(j),1); end do
    acc=acc+vl*tijk(s,ind(1:ds))
   end do; end do; end do; end do
   write(*,'(a,2i4,2es26.17)') 'marg ',k,i,marg(i,k),acc
  end do
 end do
 call dealloc(a); call dealloc(b); call dealloc(c); call dealloc(w); call dealloc(res); call dealloc(s); call dealloc(ws)
 write(*,'(a)') 'done'
end program
