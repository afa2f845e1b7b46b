! test_tijk_batch -- the generic tijk of the drop-in tt_lib at many multi-indices: tijk(tt, ind(:,:)) (dtt_ijk_many, one batched
! call on the device) next to a loop over tijk(tt, ind(:,p)), for a train built on the host (rank 3, index-dependent cores) and
! for the same train after svd.  One line per element: tag, point, batched value, looped value.
program main
 use tt_lib
 implicit none
 integer,parameter :: d=6, npts=40
 type(dtt) :: a,b,c
 integer :: ind(d,npts),k,j,p
 double precision :: vb(npts),vl
 a%l=1; a%m=d; a%n(1:d)=[4,5,3,6,4,5]; call ones(a)
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
 do p=1,npts
  do k=1,d
   ind(k,p)=1+mod(7*p+3*k+p*k,c%n(k))
  end do
 end do
 ind(:,1)=1; ind(:,2)=c%n(1:d)
 ind(3,5)=0; ind(1,9)=c%n(1)+1; ind(d,11)=-2    ! outside 1..n(k): -3 both ways
 write(*,'(a,7i3)') 'ranks ',c%r(0:d)
 vb=tijk(c,ind)
 do p=1,npts
  vl=tijk(c,ind(:,p))
  write(*,'(a,i4,2es26.17)') 'host ',p,vb(p),vl
 end do
 call svd(c,1.d-14)
 write(*,'(a,7i3)') 'ranks ',c%r(0:d)
 vb=tijk(c,ind)
 do p=1,npts
  vl=tijk(c,ind(:,p))
  write(*,'(a,i4,2es26.17)') 'svd ',p,vb(p),vl
 end do
 call dealloc(a); call dealloc(b); call dealloc(c)
 write(*,'(a)') 'done'
end program
