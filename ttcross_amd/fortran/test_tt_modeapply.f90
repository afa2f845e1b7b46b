! test_tt_modeapply -- modeapply of the drop-in tt_lib (ttx_mode_apply on the device).  Usage: test_tt_modeapply FILE [MODE]
! FILE is a train written by dtt_write.  Mode k of it gets the matrix A_k(j,i) = cos(0.3 j i + 0.1 k) - 0.25 with
! m(k) = n(k) + 1 rows where k is odd; even modes are left alone.  MODE: 0 exact (the default), 1 matrix cores.
! Lines: 'ranks' of the result; 'modes' its sizes; 'elem' p, the multi-index, the element (24 of them).
program main
 use tt_lib
 use ttio_lib
 implicit none
 integer,parameter :: npts=24
 type(dtt) :: x,res
 character(len=512) :: fnam,arg
 integer :: m(tt_size),ind(tt_size),mode,info,k,i,j,p,d,off
 double precision,allocatable :: a(:)
 double precision :: v
 if(command_argument_count().lt.1)then; write(*,'(a)') 'usage: test_tt_modeapply FILE [MODE]'; stop 2; endif
 call get_command_argument(1,fnam)
 mode=0
 if(command_argument_count().ge.2)then; call get_command_argument(2,arg); read(arg,*) mode; endif
 call read(x,trim(fnam),info)
 if(info.ne.0)then; write(*,'(a)') 'cannot read the train'; stop 3; endif
 d=x%m; m=0; off=0
 do k=1,d,2; m(k)=x%n(k)+1; off=off+m(k)*x%n(k); end do
 allocate(a(off)); off=0
 do k=1,d,2
  do i=1,x%n(k); do j=1,m(k)
   a(off+j+m(k)*(i-1))=cos(0.3d0*j*i+0.1d0*k)-0.25d0
  end do; end do
  off=off+m(k)*x%n(k)
 end do
 call modeapply(x,m(1:d),a,res,mode)
 write(*,'(a,64i4)') 'ranks ',res%r(0:d)
 write(*,'(a,64i4)') 'modes ',res%n(1:d)
 do p=1,npts
  do k=1,d; ind(k)=1+mod(p*(2*k+1)+k,res%n(k)); end do
  v=tijk(res,ind(1:d))
  write(*,'(a,i4,es26.17)') 'elem ',p,v
 end do
 call dealloc(x); call dealloc(res)
 write(*,'(a)') 'done'
end program
