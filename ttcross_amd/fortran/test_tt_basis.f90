! test_tt_basis -- basisval of the drop-in tt_lib (ttx_basis_batch on the device) for a train built on the host (rank 3,
! index-dependent cores).  'node' lines: the hat-function basis at its own nodes (mode 0) next to the batched tijk at those indices (the device's
! chain: equal) and the host's element.  'cos' lines: the cosine basis at scattered points, modes 0 and 1, next to the plain sum over all multi-indices
! sum_i tijk(i) prod_k c cos((i_k - 1) pi (x_k - a)/(b - a)) formed here and the sum of the terms' absolute values.  One line per point.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=4, npts=24
 double precision,parameter :: lo=-1.d0, hi=2.5d0, pi=3.14159265358979323846d0
 type(dtt) :: a,b,c
 integer :: ind(d,npts),i(d),k,j,p
 double precision :: x(d,npts),v0(npts),v1(npts),vb(npts),vl,va,term
 a%l=1; a%m=d; a%n(1:d)=[4,5,3,6]; call ones(a)
 b=a
 do k=1,d
  do j=1,a%n(k)
   a%u(k)%p(1,j,1)=1.d0+0.25d0*j-0.1d0*k
   b%u(k)%p(1,j,1)=cos(0.7d0*j+k)
  end do
 end do
 c=a+b
 do k=1,d; do j=1,a%n(k); a%u(k)%p(1,j,1)=sin(1.3d0*j*k)+0.2d0; end do; end do
 c=c+a                                          ! rank 3
 write(*,'(a,5i3)') 'ranks ',c%r(0:d)
 do p=1,npts
  do k=1,d
   ind(k,p)=1+mod(7*p+3*k+p*k,c%n(k))
   x(k,p)=lo+(hi-lo)*dble(ind(k,p)-1)/dble(c%n(k)-1)          ! the node itself, as basisval forms it
  end do
 end do
 call basisval(c,x,2,lo,hi,v0,0)
 vb=tijk(c,ind)                                 ! one batched call on the device
 do p=1,npts
  write(*,'(a,i4,3es26.17)') 'node ',p,v0(p),vb(p),tijk(c,ind(:,p))
 end do
 do p=1,npts
  do k=1,d; x(k,p)=lo+(hi-lo)*(0.5d0+0.5d0*sin(1.7d0*p+0.9d0*k*k)); end do
 end do
 call basisval(c,x,1,lo,hi,v0,0,.true.)
 call basisval(c,x,1,lo,hi,v1,1,.true.)
 do p=1,npts
  vl=0.d0; va=0.d0
  do j=0,product(c%n(1:d))-1
   i(1)=j
   do k=1,d; if(k.lt.d)i(k+1)=i(k)/c%n(k); i(k)=1+mod(i(k),c%n(k)); end do
   term=tijk(c,i)
   do k=1,d
    term=term*cos(dble(i(k)-1)*pi*(x(k,p)-lo)/(hi-lo)); if(i(k).eq.1)term=term*0.5d0
   end do
   vl=vl+term; va=va+abs(term)
  end do
  write(*,'(a,i4,4es26.17)') 'cos ',p,v0(p),v1(p),vl,va
 end do
 call dealloc(a); call dealloc(b); call dealloc(c)
 write(*,'(a)') 'done'
end program
