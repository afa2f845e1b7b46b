! test_tt_topk -- topk of the drop-in tt_lib: the four largest elements of the train read from the stream file given as the
! argument, one line per row: tag, the indices, val; then the bound and tijk of the first row.
program main
 use tt_lib
 use ttio_lib
 implicit none
 integer,parameter :: k=4
 type(dtt) :: a
 character(len=512) :: fin
 integer :: info,j,nf
 integer,allocatable :: ind(:,:)
 double precision :: val(k),bound
 call get_command_argument(1,fin)
 call read(a,trim(fin),info)
 if(info.ne.0)then; write(*,'(a,i4)') 'read info',info; stop 1; endif
 allocate(ind(a%m,k))
 call topk(a,k,ind,val,bound,nfound=nf)
 write(*,'(a,i4)') 'nfound',nf
 do j=1,nf
  write(*,'(a,*(1x,i0))',advance='no') 'row',ind(:,j)
  write(*,'(1x,es26.17)') val(j)
 end do
 write(*,'(a,es26.17)') 'bound',bound
 write(*,'(a,es26.17)') 'tijk ',tijk(a,ind(:,1))
 call dealloc(a)
 write(*,'(a)') 'done'
end program
