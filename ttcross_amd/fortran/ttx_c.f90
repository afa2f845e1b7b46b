! ttx_c.f90 -- ISO_C_BINDING view of include/ttx.h (the C-ABI of libttx.so).
! This is the binding a maintainer of the reference adds to call the MI355X engine from lib/dmrgg.f90.
module ttx_c
 use iso_c_binding
 implicit none
 integer(c_int32_t),parameter :: TTX_FUN_ISING=1, TTX_FUN_STDNORM=2, TTX_FUN_MVN=3, TTX_FUN_HOST=4, TTX_FUN_COSCOEFF=5, TTX_FUN_DEVICE=6, TTX_FUN_TRAINS=7
 integer(c_int32_t),parameter :: TTX_TRAINS_MAX=8, TTX_TOP_PRODUCT=1, TTX_TOP_RATIO=2, TTX_TOP_SQRTABS=3, TTX_TOP_DEVICE=4
 integer(c_int32_t),parameter :: TTX_BASIS_COS=1, TTX_BASIS_LINEAR=2, TTX_BASIS_HALVE_FIRST=1
 type,bind(C) :: ttx_basis_t            ! ttx_basis: one mode's basis; nodes = c_loc of n(k) ascending nodes (LINEAR) or c_null_ptr
  integer(c_int32_t) :: kind,flags
  real(c_double) :: a,b
  type(c_ptr) :: nodes
 end type
 type,bind(C) :: ttx_config
  integer(c_int32_t) :: d
  type(c_ptr) :: n
  integer(c_int32_t) :: fun_id
  type(c_ptr) :: par
  integer(c_int32_t) :: npar
  type(c_ptr) :: aux
  integer(c_int32_t) :: naux
  type(c_ptr) :: quadw
  real(c_double) :: accuracy
  integer(c_int32_t) :: maxrank
  integer(c_int32_t) :: pivoting
  real(c_double) :: tru
  integer(c_int32_t) :: has_tru
  integer(c_int32_t) :: nproc
  type(c_ptr) :: mybonds
  integer(c_int32_t) :: device
  integer(c_int32_t) :: world_rank
  integer(c_int32_t) :: world_size
  integer(c_int32_t) :: verbose
  integer(c_int32_t) :: arith
 end type
 interface
  function ttx_last_error() bind(C,name='ttx_last_error') result(p)
   import; type(c_ptr) :: p
  end function
  function ttx_create(h,cfg) bind(C,name='ttx_create') result(rc)
   import; type(c_ptr),intent(out) :: h; type(ttx_config),intent(in) :: cfg; integer(c_int) :: rc
  end function
  subroutine ttx_destroy(h) bind(C,name='ttx_destroy')
   import; type(c_ptr),value :: h
  end subroutine
  function ttx_set_integrand_host(h,fun,par) bind(C,name='ttx_set_integrand_host') result(rc)   ! the user's `fun`, lib/dmrgg.f90:18
   import; type(c_ptr),value :: h; type(c_funptr),value :: fun; type(c_ptr),value :: par; integer(c_int) :: rc
  end function
  ! the user's `fun` on the device: a code object written against include/ttx_device_fun.h (the engine COPIES par)
  function ttx_set_integrand_device(h,image,nbytes,name,par,npar) bind(C,name='ttx_set_integrand_device') result(rc)
   import; type(c_ptr),value :: h; type(c_ptr),value :: image; integer(c_int64_t),value :: nbytes; character(kind=c_char) :: name(*)
   type(c_ptr),value :: par; integer(c_int32_t),value :: npar; integer(c_int) :: rc
  end function
  function ttx_set_integrand_device_file(h,path,name,par,npar) bind(C,name='ttx_set_integrand_device_file') result(rc)
   import; type(c_ptr),value :: h; character(kind=c_char) :: path(*),name(*); type(c_ptr),value :: par; integer(c_int32_t),value :: npar
   integer(c_int) :: rc
  end function
  ! integrand of resident trains (TTX_FUN_TRAINS, include/ttx.h): x = m engine handles
  function ttx_set_integrand_trains(h,m,x,op) bind(C,name='ttx_set_integrand_trains') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),value :: m,op; type(c_ptr),intent(in) :: x(*); integer(c_int) :: rc
  end function
  function ttx_set_integrand_trains_device_file(h,m,x,path,name,par,npar) bind(C,name='ttx_set_integrand_trains_device_file') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),value :: m; type(c_ptr),intent(in) :: x(*); character(kind=c_char) :: path(*),name(*)
   type(c_ptr),value :: par; integer(c_int32_t),value :: npar; integer(c_int) :: rc
  end function
  function ttx_trainfun_last(h,ms,launches,elements) bind(C,name='ttx_trainfun_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms; integer(c_int64_t),intent(out) :: launches,elements; integer(c_int) :: rc
  end function
  function ttx_eval_device(h,npts,ind,out) bind(C,name='ttx_eval_device') result(rc)
   import; type(c_ptr),value :: h; integer(c_int64_t),value :: npts; integer(c_int32_t) :: ind(*); real(c_double) :: out(*); integer(c_int) :: rc
  end function
  function ttx_getppid() bind(C,name='getppid') result(p)      ! libc: the launcher's pid, shared by the ranks of a job
   import; integer(c_int) :: p
  end function
  function ttx_usleep(us) bind(C,name='usleep') result(rc)
   import; integer(c_int32_t),value :: us; integer(c_int) :: rc
  end function
  function ttx_fun_id(h) bind(C,name='ttx_fun_id') result(id)
   import; type(c_ptr),value :: h; integer(c_int) :: id
  end function
  function ttx_host_calls(h) bind(C,name='ttx_host_calls') result(n)
   import; type(c_ptr),value :: h; integer(c_int64_t) :: n
  end function
  function ttx_comm_unique_id(id) bind(C,name='ttx_comm_unique_id') result(rc)   ! replaces mpi_init, test_crs_ising.f90:31-36
   import; integer(c_int8_t) :: id(128); integer(c_int) :: rc
  end function
  function ttx_comm_init(h,id) bind(C,name='ttx_comm_init') result(rc)
   import; type(c_ptr),value :: h; integer(c_int8_t) :: id(128); integer(c_int) :: rc
  end function
  function ttx_comm_init_shm(h,name) bind(C,name='ttx_comm_init_shm') result(rc)   ! node-local host transport (several ranks on one GPU, no MPI)
   import; type(c_ptr),value :: h; character(kind=c_char) :: name(*); integer(c_int) :: rc
  end function
  function ttx_run(h) bind(C,name='ttx_run') result(rc)
   import; type(c_ptr),value :: h; integer(c_int) :: rc
  end function
  function ttx_neval(h) bind(C,name='ttx_neval') result(n)
   import; type(c_ptr),value :: h; integer(c_int64_t) :: n
  end function
  function ttx_get_ranks(h,r) bind(C,name='ttx_get_ranks') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),intent(out) :: r(*); integer(c_int) :: rc
  end function
  function ttx_core_size(h,k) bind(C,name='ttx_core_size') result(n)
   import; type(c_ptr),value :: h; integer(c_int),value :: k; integer(c_int64_t) :: n
  end function
  function ttx_get_core(h,k,buf) bind(C,name='ttx_get_core') result(rc)
   import; type(c_ptr),value :: h; integer(c_int),value :: k; real(c_double),intent(out) :: buf(*); integer(c_int) :: rc
  end function
  function ttx_quad(h,w,val) bind(C,name='ttx_quad') result(rc)
   import; type(c_ptr),value :: h; type(c_ptr),value :: w; real(c_double),intent(out) :: val; integer(c_int) :: rc
  end function
  function ttx_ort(h) bind(C,name='ttx_ort') result(rc)
   import; type(c_ptr),value :: h; integer(c_int) :: rc
  end function
  function ttx_svd(h,tol,rmax) bind(C,name='ttx_svd') result(rc)
   import; type(c_ptr),value :: h; real(c_double),value :: tol; integer(c_int32_t),value :: rmax; integer(c_int) :: rc
  end function
  function ttx_norm(h,tol,val) bind(C,name='ttx_norm') result(rc)
   import; type(c_ptr),value :: h; real(c_double),value :: tol; real(c_double),intent(out) :: val; integer(c_int) :: rc
  end function
  function ttx_lognrm(h,tol,val) bind(C,name='ttx_lognrm') result(rc)
   import; type(c_ptr),value :: h; real(c_double),value :: tol; real(c_double),intent(out) :: val; integer(c_int) :: rc
  end function
  function ttx_dot(hx,hy,val) bind(C,name='ttx_dot') result(rc)
   import; type(c_ptr),value :: hx,hy; real(c_double),intent(out) :: val; integer(c_int) :: rc
  end function
  function ttx_ijk(h,ind,val) bind(C,name='ttx_ijk') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),intent(in) :: ind(*); real(c_double),intent(out) :: val; integer(c_int) :: rc
  end function
  ! the train at a batch of multi-indices / coordinate vectors (include/ttx.h); mode: 0 exact, 1 MFMA, 2 auto
  function ttx_ijk_batch(h,npts,ind,out,mode) bind(C,name='ttx_ijk_batch') result(rc)
   import; type(c_ptr),value :: h; integer(c_int64_t),value :: npts; integer(c_int32_t),intent(in) :: ind(*)
   real(c_double),intent(out) :: out(*); integer(c_int32_t),value :: mode; integer(c_int) :: rc
  end function
  function ttx_ijk_batch_dev(h,npts,ind_dev,out_dev,mode) bind(C,name='ttx_ijk_batch_dev') result(rc)
   import; type(c_ptr),value :: h,ind_dev,out_dev; integer(c_int64_t),value :: npts; integer(c_int32_t),value :: mode; integer(c_int) :: rc
  end function
  function ttx_value_batch(h,npts,dd,x,out,mode) bind(C,name='ttx_value_batch') result(rc)
   import; type(c_ptr),value :: h; integer(c_int64_t),value :: npts; integer(c_int32_t),value :: dd,mode
   real(c_double),intent(in) :: x(*); real(c_double),intent(out) :: out(*); integer(c_int) :: rc
  end function
  ! chosen modes of the train contracted with rank-1 weights (include/ttx.h); w: d blocks of n(k) weights or c_null_ptr (ones)
  function ttx_contract(h,keep,w,out) bind(C,name='ttx_contract') result(rc)
   import; type(c_ptr),value :: h,w; integer(c_int32_t),intent(in) :: keep(*); type(c_ptr) :: out; integer(c_int) :: rc
  end function
  function ttx_marginals(h,w,out) bind(C,name='ttx_marginals') result(rc)
   import; type(c_ptr),value :: h,w; real(c_double),intent(out) :: out(*); integer(c_int) :: rc
  end function
  ! sums and elementwise products of resident trains (include/ttx.h): out is a new engine owned by the caller
  function ttx_lincomb(m,coef,x,out) bind(C,name='ttx_lincomb') result(rc)
   import; integer(c_int32_t),value :: m; real(c_double),intent(in) :: coef(*); type(c_ptr),intent(in) :: x(*); type(c_ptr) :: out; integer(c_int) :: rc
  end function
  function ttx_hadamard(x,y,out) bind(C,name='ttx_hadamard') result(rc)
   import; type(c_ptr),value :: x,y; type(c_ptr) :: out; integer(c_int) :: rc
  end function
  function ttx_algebra_last(h,ms,bytes_read,bytes_written) bind(C,name='ttx_algebra_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms,bytes_read,bytes_written; integer(c_int) :: rc
  end function
  ! a rounded sum of resident trains (include/ttx.h): rsketch 0 = 128, tol < 0 = no truncation, rmax 0 = absent, mode 0 / 1 / 2
  function ttx_lincomb_round(m,coef,x,rsketch,tol,rmax,seed,mode,out) bind(C,name='ttx_lincomb_round') result(rc)
   import; integer(c_int32_t),value :: m,rsketch,rmax,mode; real(c_double),intent(in) :: coef(*); type(c_ptr),intent(in) :: x(*)
   real(c_double),value :: tol; integer(c_int64_t),value :: seed; type(c_ptr) :: out; integer(c_int) :: rc
  end function
  ! matrices applied to chosen modes (include/ttx.h): a = the column-major blocks m(k) x n(k) of the applied modes, one after the other
  function ttx_mode_apply(h,m,a,mode,out) bind(C,name='ttx_mode_apply') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),intent(in) :: m(*); real(c_double),intent(in) :: a(*); integer(c_int32_t),value :: mode
   type(c_ptr) :: out; integer(c_int) :: rc
  end function
  function ttx_mode_apply_last(h,ms,bytes_read,bytes_written,flops,mode_ran) bind(C,name='ttx_mode_apply_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms,bytes_read,bytes_written,flops; integer(c_int32_t),intent(out) :: mode_ran; integer(c_int) :: rc
  end function
  ! the train in a function basis at real points (include/ttx.h): x(d,npts), basis(d) of type ttx_basis_t; mode 0 / 1 / 2
  function ttx_basis_batch(h,npts,x,basis,out,mode) bind(C,name='ttx_basis_batch') result(rc)
   import; type(c_ptr),value :: h; integer(c_int64_t),value :: npts; real(c_double),intent(in) :: x(*); type(ttx_basis_t),intent(in) :: basis(*)
   real(c_double),intent(out) :: out(*); integer(c_int32_t),value :: mode; integer(c_int) :: rc
  end function
  function ttx_basis_last(h,ms_table,ms_chain,flops,mode_ran) bind(C,name='ttx_basis_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_table,ms_chain,flops; integer(c_int32_t),intent(out) :: mode_ran; integer(c_int) :: rc
  end function
  ! samples drawn from the resident train (include/ttx.h); u(d,npts), ind(d,npts); w, fixed, logq, val: c_null_ptr where not wanted
  function ttx_sample(h,npts,u,w,fixed,ind,logq,val) bind(C,name='ttx_sample') result(rc)
   import; type(c_ptr),value :: h,w,fixed,logq,val; integer(c_int64_t),value :: npts; real(c_double),intent(in) :: u(*)
   integer(c_int32_t),intent(out) :: ind(*); integer(c_int) :: rc
  end function
  function ttx_sample_dev(h,npts,u,w,fixed,ind,logq,val) bind(C,name='ttx_sample_dev') result(rc)
   import; type(c_ptr),value :: h,u,w,fixed,ind,logq,val; integer(c_int64_t),value :: npts; integer(c_int) :: rc
  end function
  function ttx_sample_last(h,ms_head,bytes_head,ms_draw,nfailed) bind(C,name='ttx_sample_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_head,bytes_head,ms_draw; integer(c_int64_t),intent(out) :: nfailed; integer(c_int) :: rc
  end function
  ! samples drawn from the square of the resident train (include/ttx.h); as ttx_sample, with gamma and mode by value
  function ttx_sample_sq(h,npts,u,w,fixed,gamma,mode,ind,logq,val) bind(C,name='ttx_sample_sq') result(rc)
   import; type(c_ptr),value :: h,w,fixed,logq,val; integer(c_int64_t),value :: npts; real(c_double),intent(in) :: u(*)
   real(c_double),value :: gamma; integer(c_int32_t),value :: mode; integer(c_int32_t),intent(out) :: ind(*); integer(c_int) :: rc
  end function
  function ttx_sample_sq_dev(h,npts,u,w,fixed,gamma,mode,ind,logq,val) bind(C,name='ttx_sample_sq_dev') result(rc)
   import; type(c_ptr),value :: h,u,w,fixed,ind,logq,val; integer(c_int64_t),value :: npts; real(c_double),value :: gamma
   integer(c_int32_t),value :: mode; integer(c_int) :: rc
  end function
  function ttx_sample_sq_last(h,ms_head,ms_rows,ms_pick,flops,nfailed,mode_ran) bind(C,name='ttx_sample_sq_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_head,ms_rows,ms_pick,flops; integer(c_int64_t),intent(out) :: nfailed
   integer(c_int32_t),intent(out) :: mode_ran; integer(c_int) :: rc
  end function
  ! real-valued samples from the interpolant of the resident train (include/ttx.h); u(d,npts), x(d,npts), nodes(d) = the addresses
  ! of the node rows; cond, cell, logq, val: c_null_ptr where not wanted
  function ttx_sample_real(h,npts,u,nodes,cond,x,cell,logq,val) bind(C,name='ttx_sample_real') result(rc)
   import; type(c_ptr),value :: h,cond,cell,logq,val; integer(c_int64_t),value :: npts; real(c_double),intent(in) :: u(*)
   type(c_ptr),intent(in) :: nodes(*); real(c_double),intent(out) :: x(*); integer(c_int) :: rc
  end function
  function ttx_sample_real_dev(h,npts,u,nodes,cond,x,cell,logq,val) bind(C,name='ttx_sample_real_dev') result(rc)
   import; type(c_ptr),value :: h,u,cond,x,cell,logq,val; integer(c_int64_t),value :: npts; type(c_ptr),intent(in) :: nodes(*); integer(c_int) :: rc
  end function
  function ttx_sample_real_last(h,ms_head,bytes_head,ms_draw,nfailed) bind(C,name='ttx_sample_real_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_head,bytes_head,ms_draw; integer(c_int64_t),intent(out) :: nfailed; integer(c_int) :: rc
  end function
  ! real-valued samples from the square of the interpolant of the resident train (include/ttx.h); as ttx_sample_real, with gamma and
  ! mode by value
  function ttx_sample_sq_real(h,npts,u,nodes,cond,gamma,mode,x,cell,logq,val) bind(C,name='ttx_sample_sq_real') result(rc)
   import; type(c_ptr),value :: h,cond,cell,logq,val; integer(c_int64_t),value :: npts; real(c_double),intent(in) :: u(*)
   type(c_ptr),intent(in) :: nodes(*); real(c_double),value :: gamma; integer(c_int32_t),value :: mode; real(c_double),intent(out) :: x(*); integer(c_int) :: rc
  end function
  function ttx_sample_sq_real_dev(h,npts,u,nodes,cond,gamma,mode,x,cell,logq,val) bind(C,name='ttx_sample_sq_real_dev') result(rc)
   import; type(c_ptr),value :: h,u,cond,x,cell,logq,val; integer(c_int64_t),value :: npts; type(c_ptr),intent(in) :: nodes(*)
   real(c_double),value :: gamma; integer(c_int32_t),value :: mode; integer(c_int) :: rc
  end function
  function ttx_sample_sq_real_last(h,ms_head,ms_rows,ms_pick,flops,nfailed,mode_ran) bind(C,name='ttx_sample_sq_real_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_head,ms_rows,ms_pick,flops; integer(c_int64_t),intent(out) :: nfailed
   integer(c_int32_t),intent(out) :: mode_ran; integer(c_int) :: rc
  end function
  ! the way back of ttx_sample_sq_real (include/ttx.h): the points x in, the uniforms u out
  function ttx_rosenblatt_sq_real(h,npts,x,nodes,cond,gamma,mode,u,cell,logq,val) bind(C,name='ttx_rosenblatt_sq_real') result(rc)
   import; type(c_ptr),value :: h,cond,cell,logq,val; integer(c_int64_t),value :: npts; real(c_double),intent(in) :: x(*)
   type(c_ptr),intent(in) :: nodes(*); real(c_double),value :: gamma; integer(c_int32_t),value :: mode; real(c_double),intent(out) :: u(*); integer(c_int) :: rc
  end function
  function ttx_rosenblatt_sq_real_dev(h,npts,x,nodes,cond,gamma,mode,u,cell,logq,val) bind(C,name='ttx_rosenblatt_sq_real_dev') result(rc)
   import; type(c_ptr),value :: h,x,cond,u,cell,logq,val; integer(c_int64_t),value :: npts; type(c_ptr),intent(in) :: nodes(*)
   real(c_double),value :: gamma; integer(c_int32_t),value :: mode; integer(c_int) :: rc
  end function
  function ttx_rosenblatt_sq_real_last(h,ms_head,ms_rows,ms_cdf,flops,nfailed,mode_ran) bind(C,name='ttx_rosenblatt_sq_real_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_head,ms_rows,ms_cdf,flops; integer(c_int64_t),intent(out) :: nfailed
   integer(c_int32_t),intent(out) :: mode_ran; integer(c_int) :: rc
  end function
  ! the largest elements of the resident train (include/ttx.h); ind(d,K), val(K); fixed: c_null_ptr where not wanted
  function ttx_topk(h,k,which,fixed,mode,nfound,ind,val,bound) bind(C,name='ttx_topk') result(rc)
   import; type(c_ptr),value :: h,fixed; integer(c_int32_t),value :: k,which,mode; integer(c_int32_t),intent(out) :: nfound,ind(*)
   real(c_double),intent(out) :: val(*),bound; integer(c_int) :: rc
  end function
  function ttx_topk_last(h,ms_gram,ms_score,ms_select,flops,mode_ran) bind(C,name='ttx_topk_last') result(rc)
   import; type(c_ptr),value :: h; real(c_double),intent(out) :: ms_gram,ms_score,ms_select,flops; integer(c_int32_t),intent(out) :: mode_ran; integer(c_int) :: rc
  end function
  function ttx_accchk(h,nlot,einf,efro,ainf,afro,pivot) bind(C,name='ttx_accchk') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),value :: nlot; real(c_double),intent(out) :: einf,efro,ainf,afro
   integer(c_int32_t),intent(out) :: pivot(*); integer(c_int) :: rc
  end function
  function ttx_zquad(h,nf,w,out) bind(C,name='ttx_zquad') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t),value :: nf; real(c_double) :: w(*),out(*); integer(c_int) :: rc
  end function
  function ttx_from_tt(h,d,n,r,cores,device) bind(C,name='ttx_from_tt') result(rc)
   import; type(c_ptr) :: h; integer(c_int32_t),value :: d,device; integer(c_int32_t) :: n(*),r(*); real(c_double) :: cores(*); integer(c_int) :: rc
  end function
  function ttx_write(h,path) bind(C,name='ttx_write') result(rc)
   import; type(c_ptr),value :: h; character(kind=c_char) :: path(*); integer(c_int) :: rc
  end function
  function ttx_read(h,path,device) bind(C,name='ttx_read') result(rc)
   import; type(c_ptr) :: h; character(kind=c_char) :: path(*); integer(c_int32_t),value :: device; integer(c_int) :: rc
  end function
  function ttx_get_modes(h,d,n) bind(C,name='ttx_get_modes') result(rc)
   import; type(c_ptr),value :: h; integer(c_int32_t) :: d; integer(c_int32_t) :: n(*); integer(c_int) :: rc
  end function
 end interface
contains
 subroutine ttx_warn(who)
  ! print the engine's last error without stopping (the reference's I/O routines report and return, lib/ttio.f90:85-108)
  character(len=*),intent(in) :: who
  character(kind=c_char),pointer :: s(:)
  integer :: i
  call c_f_pointer(ttx_last_error(),s,[512])
  write(*,'(a,a)',advance='no') who,': '
  do i=1,512
   if(s(i).eq.c_null_char)exit
   write(*,'(a)',advance='no') s(i)
  end do
  write(*,*)
 end subroutine
 subroutine ttx_check(rc,who)
  ! the reference reports errors as `write(*,*) ...; stop` (e.g. lib/dmrgg.f90:88-91,105-117)
  integer(c_int),intent(in) :: rc
  character(len=*),intent(in) :: who
  character(kind=c_char),pointer :: s(:)
  integer :: i
  if(rc.eq.0)return
  call c_f_pointer(ttx_last_error(),s,[512])
  write(*,'(a,a)',advance='no') who,': '
  do i=1,512
   if(s(i).eq.c_null_char)exit
   write(*,'(a)',advance='no') s(i)
  end do
  write(*,*)
  stop 1
 end subroutine
end module
