! test_tt_roundsum -- roundsum of the drop-in tt_lib (ttx_lincomb_round on the device).  Usage: test_tt_roundsum FILE1 FILE2 FILE3
! The files are trains of equal modes written by dtt_write.  res = 1.5 x1 - 0.5 x2 + 0.25 x3 with rank=17, seed=5, no truncation;
! the first train is passed as a host train (its handle dropped, so that it is staged), the others resident.
! Lines: 'ranks' of the result; 'elem' p, the element at the p-th multi-index (24 of them); then the same sum with tol=1d-10:
! 'trunc' and its ranks.
program main
 use tt_lib
 use ttio_lib
 use iso_c_binding, only: c_null_ptr
 use ttx_c, only: ttx_destroy
 implicit none
 integer,parameter :: npts=24
 type(dtt) :: x(3),res,cut
 character(len=512) :: fnam
 integer :: ind(tt_size),info,k,p,d,t
 double precision :: v
 if(command_argument_count().lt.3)then; write(*,'(a)') 'usage: test_tt_roundsum FILE1 FILE2 FILE3'; stop 2; endif
 do t=1,3
  call get_command_argument(t,fnam)
  call read(x(t),trim(fnam),info)
  if(info.ne.0)then; write(*,'(a)') 'cannot read a train'; stop 3; endif
 end do
 call ttx_destroy(x(1)%ttx); x(1)%ttx=c_null_ptr
 d=x(1)%m
 call roundsum([1.5d0,-0.5d0,0.25d0],x,res,rank=17,seed=5)
 write(*,'(a,64i4)') 'ranks ',res%r(0:d)
 do p=1,npts
  do k=1,d; ind(k)=1+mod(p*(2*k+1)+k,res%n(k)); end do
  v=tijk(res,ind(1:d))
  write(*,'(a,i4,es26.17)') 'elem ',p,v
 end do
 call roundsum([1.5d0,-0.5d0,0.25d0],x,cut,rank=17,tol=1d-10,seed=5)
 write(*,'(a,64i4)') 'trunc ',cut%r(0:d)
 do t=1,3; call dealloc(x(t)); end do
 call dealloc(res); call dealloc(cut)
 write(*,'(a)') 'done'
end program
