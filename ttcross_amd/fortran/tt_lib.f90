! tt_lib.f90 -- drop-in subset of the reference's ptype_lib / tt_lib (lib/ptype.f90:4-6, lib/tt.f90:16-37,
! 879-892, 908-916, 1228-1245, 1348-1360): the dtt container the drivers and dtt_dmrgg exchange.
! Same component names; one extra hidden component carries the device-engine handle.
module ptype_lib
 implicit none
 type,public :: pointd3
  double precision,dimension(:,:,:),pointer,contiguous :: p=>null()
 end type
 type,public :: pointz3
  double complex,dimension(:,:,:),pointer,contiguous :: p=>null()
 end type
end module

module tt_lib
 use iso_c_binding
 use ptype_lib
 implicit none
 integer,parameter :: tt_size=2048
 type,public :: dtt
  integer :: l=1
  integer :: m=0
  integer :: n(tt_size)=0
  integer :: q(tt_size)=0
  integer :: s(tt_size)=0
  integer :: t=0
  integer :: r(0:tt_size)=0
  type(pointd3) :: u(tt_size)
  type(c_ptr) :: ttx=c_null_ptr      ! engine handle after dtt_dmrgg (not in the reference)
 end type
 ! complex train (lib/tt.f90:38-52): host cores as in the reference; a ztt made from a dtt (tt_z = tt) also BORROWS
 ! the device train of that dtt -- ztt_quad works on it -- and never releases it
 type,public :: ztt
  integer :: l=1
  integer :: m=0
  integer :: n(tt_size)=0
  integer :: q(tt_size)=0
  integer :: s(tt_size)=0
  integer :: t=0
  integer :: r(0:tt_size)=0
  type(pointz3) :: u(tt_size)
  type(c_ptr) :: ttx=c_null_ptr
 end type
 interface alloc;   module procedure dtt_alloc,ztt_alloc;     end interface
 interface dealloc; module procedure dtt_dealloc,ztt_dealloc; end interface
 interface assignment (=); module procedure dtt_assign,ztt_assign,ztt_dtt_assign; end interface
 interface ones;    module procedure dtt_ones;    end interface
 interface zeros;   module procedure dtt_zeros;   end interface
 interface erank;   module procedure dtt_rank;    end interface
 ! host-side generics of lib/tt.f90:54-124 (they work on the host cores arg%u(k)%p, as in the reference)
 interface copy;    module procedure dtt_copy;    end interface
 interface ready;   module procedure dtt_ready;   end interface
 interface numel;   module procedure dtt_numel;   end interface
 interface memory;  module procedure dtt_mem;     end interface
 interface say;     module procedure dtt_say;     end interface
 interface sumall;  module procedure dtt_sumall;  end interface
 interface value;   module procedure dtt_value,dtt_value0; end interface
 interface elem;    module procedure dtt_elem;    end interface
 interface lognrm;  module procedure dtt_lognrm;  end interface
 interface operator (+); module procedure dtt_plus_dtt,dtt_plus_d; end interface
 interface operator (*); module procedure dtt_mul_dt; end interface
 ! utilities that run on the tensor train resident on the device after dtt_dmrgg (lib/tt.f90:54-124 generics)
 interface ort;         module procedure dtt_ort;  end interface
 interface svd;         module procedure dtt_svd;  end interface
 interface norm;        module procedure dtt_norm; end interface
 interface dot_product; module procedure dtt_dot;  end interface
 interface tijk;        module procedure dtt_ijk,dtt_ijk_many;  end interface
 ! partial contraction on the device (not in the reference): contract(arg,keep,res,w), marginals(arg,marg,w)
 interface contract;    module procedure dtt_contract;  end interface
 interface marginals;   module procedure dtt_marginals; end interface
 ! matrices applied to chosen modes on the device (not in the reference): modeapply(arg,m,a,res,mode)
 interface modeapply;   module procedure dtt_modeapply; end interface
 ! the train in a function basis at real points on the device (not in the reference): basisval(arg,x,kind,a,b,res,mode,halve)
 interface basisval;    module procedure dtt_basisval; end interface
 ! samples drawn from the train on the device (not in the reference): sample(arg,u,ind,w,fixed,logq,val)
 interface sample;      module procedure dtt_sample;    end interface
 ! real points drawn from the piecewise-linear interpolant of the train on the device (not in the reference):
 ! sample_real(arg,u,nodes,x,cond,cell,logq,val)
 interface sample_real; module procedure dtt_sample_real; end interface
 ! samples from the square of the train, the squared-density sampler: sample_sq(arg,u,ind,w,fixed,gamma,mode,logq,val)
 interface sample_sq;   module procedure dtt_sample_sq;   end interface
 ! real points from the square of the interpolant: sample_sq_real(arg,u,nodes,x,cond,gamma,mode,cell,logq,val)
 interface sample_sq_real; module procedure dtt_sample_sq_real; end interface
 ! the way back: the uniforms of given points under sample_sq_real's proposal: rosenblatt_sq_real(arg,x,nodes,u,cond,gamma,mode,cell,logq,val)
 interface rosenblatt_sq_real; module procedure dtt_rosenblatt_sq_real; end interface
 ! the largest elements of the train with a bound on the rest, on the device (not in the reference): topk(arg,k,ind,val,bound,which,fixed,mode)
 interface topk;        module procedure dtt_topk;      end interface
 ! sums and elementwise products on the device (not in the reference; its host + and * above stay as they are):
 ! axpby(alpha,x,beta,y) = alpha*x + beta*y, hadamard(x,y) = x(i)*y(i).  Both return a dtt that holds the new train on the device
 ! and, pulled, in %u; the variable the result is assigned to takes the device train over (dtt_assign)
 interface axpby;       module procedure dtt_axpby;    end interface
 ! roundsum(c,x,res,rank,tol,rmax,seed): res = sum_t c(t) x(t) rounded on the device by a randomized sketch (ttx_lincomb_round)
 interface roundsum;    module procedure dtt_roundsum; end interface
 interface hadamard;    module procedure dtt_hadamard; end interface
 type(c_ptr),private,save :: tt_pending=c_null_ptr      ! the device train of the last axpby / hadamard result, until it is assigned
contains
 subroutine dtt_result(res,hn,arg)
  ! res = the new device train hn with the modes of arg, pulled.  A function result cannot be dealloc'ed by the caller: its
  ! device train goes to the variable it is assigned to; one that never was assigned is released by the next result
  use ttx_c
  type(dtt),intent(inout) :: res
  type(c_ptr),intent(in) :: hn
  type(dtt),intent(in) :: arg
  if(c_associated(tt_pending))call ttx_destroy(tt_pending)
  res%l=1; res%m=arg%m; res%n(1:arg%m)=arg%n(1:arg%m)
  res%ttx=hn; call dtt_pull(res); tt_pending=hn
 end subroutine
 function dtt_axpby(alpha,x,beta,y) result(c)
  ! c = alpha*x + beta*y in one call on the device (ttx_lincomb): the cores of the host alpha*x + beta*y bit for bit -- the same
  ! block layout, the same single multiply of the first cores; host trains are staged for the call like for norm / dot_product
  use ttx_c
  double precision,intent(in) :: alpha,beta
  type(dtt),intent(in) :: x,y
  type(dtt) :: c
  type(c_ptr) :: hs(2),hn
  real(c_double) :: cf(2)
  logical :: tx,ty
  call dtt_stage(x,hs(1),tx,'dtt_axpby'); call dtt_stage(y,hs(2),ty,'dtt_axpby')
  cf(1)=alpha; cf(2)=beta; hn=c_null_ptr
  call ttx_check(ttx_lincomb(2_c_int32_t,cf,hs,hn),'dtt_axpby')
  if(tx)call ttx_destroy(hs(1))
  if(ty)call ttx_destroy(hs(2))
  call dtt_result(c,hn,x)
 end function
 subroutine dtt_roundsum(c,x,res,rank,tol,rmax,seed)
  ! res = sum_t c(t) x(t), rounded on the device in one call (ttx_lincomb_round): no core of rank sum_t r_t is formed, so the sum may
  ! go far beyond the rank 128 that axpby and + stop at.  rank: the sketch rank (absent or 0: 128); tol: absent or negative keeps the
  ! left-orthogonal train with the sketch ranks, tol >= 0 truncates it as svd(res,tol,rmax) does; seed: the sketch's (default 0).
  ! Host trains are staged for the call like for axpby.  res holds the new train on the device and, pulled, in res%u.
  use ttx_c
  double precision,intent(in) :: c(:)
  type(dtt),intent(in) :: x(:)
  type(dtt),intent(inout) :: res
  integer,intent(in),optional :: rank,rmax,seed
  double precision,intent(in),optional :: tol
  type(c_ptr),allocatable :: hs(:)
  logical,allocatable :: tmp(:)
  real(c_double),allocatable :: cf(:)
  type(c_ptr) :: hn
  integer(c_int32_t) :: rk,rm
  integer(c_int64_t) :: sd
  real(c_double) :: tl
  integer :: t,m
  m=size(x)
  if(m.lt.1 .or. size(c).ne.m)then;write(*,*)'dtt_roundsum: one coefficient per train expected; got ',size(c),m;stop;endif
  call dtt_dealloc(res)
  rk=0; if(present(rank))rk=rank
  rm=0; if(present(rmax))rm=rmax
  sd=0; if(present(seed))sd=seed
  tl=-1.d0; if(present(tol))tl=tol
  allocate(hs(m),tmp(m),cf(m)); cf=c
  do t=1,m; call dtt_stage(x(t),hs(t),tmp(t),'dtt_roundsum'); end do
  hn=c_null_ptr
  call ttx_check(ttx_lincomb_round(int(m,c_int32_t),cf,hs,rk,tl,rm,sd,2_c_int32_t,hn),'dtt_roundsum')
  do t=1,m; if(tmp(t))call ttx_destroy(hs(t)); end do
  res%l=1; res%m=x(1)%m; res%n(1:res%m)=x(1)%n(1:res%m)
  res%ttx=hn; call dtt_pull(res)
 end subroutine
 function dtt_hadamard(x,y) result(c)
  ! c(i) = x(i)*y(i) in one call on the device (ttx_hadamard): ranks multiply, the index of x runs fastest on both bonds
  use ttx_c
  type(dtt),intent(in) :: x,y
  type(dtt) :: c
  type(c_ptr) :: hx,hy,hn
  logical :: tx,ty
  call dtt_stage(x,hx,tx,'dtt_hadamard'); call dtt_stage(y,hy,ty,'dtt_hadamard')
  hn=c_null_ptr
  call ttx_check(ttx_hadamard(hx,hy,hn),'dtt_hadamard')
  if(tx)call ttx_destroy(hx)
  if(ty)call ttx_destroy(hy)
  call dtt_result(c,hn,x)
 end function
 subroutine ztt_alloc(arg)
  type(ztt),intent(inout) :: arg
  integer :: k,ierr
  if(arg%m < arg%l) return
  do k = arg%l, arg%m
   if(associated(arg%u(k)%p)) deallocate(arg%u(k)%p)
   allocate(arg%u(k)%p(arg%r(k-1), arg%n(k), arg%r(k)), stat=ierr)
   if(ierr /= 0) then
    write(*,*) 'TT allocate fail: no memory'; stop
   end if
  end do
 end subroutine
 subroutine ztt_dealloc(arg)
  type(ztt),intent(inout) :: arg
  integer :: k
  do k = 1, tt_size
   if(associated(arg%u(k)%p)) then
    deallocate(arg%u(k)%p); nullify(arg%u(k)%p)
   end if
  end do
  arg%ttx = c_null_ptr               ! borrowed, see the type
 end subroutine
 subroutine ztt_dtt_assign(z,d)
  ! lib/tt.f90:1033-1045: complex copy of a real train (plus the borrowed device handle)
  type(ztt),intent(inout) :: z
  type(dtt),intent(in) :: d
  integer :: k
  if(d%l > d%m) then
   write(*,*) 'ztt_dtt_assign: l,m: ',d%l,d%m; return
  end if
  z%l = d%l; z%m = d%m; z%n = d%n; z%r = d%r
  call ztt_alloc(z)
  do k = d%l, d%m
   z%u(k)%p = dcmplx(d%u(k)%p, 0.d0)
  end do
  z%ttx = d%ttx
 end subroutine
 subroutine dtt_alloc(arg)
  ! (re)allocate every core k = l..m with the shape (r(k-1), n(k), r(k))
  type(dtt),intent(inout) :: arg
  integer :: k,ierr
  if(arg%m < arg%l) return
  if(arg%l < 1) then
   write(*,*) 'dtt_alloc: %l should be > 0'; stop
  end if
  if(arg%m > tt_size) then
   write(*,*) 'dtt_alloc: %m exceeds tt_size, change parameter and recompile!'; stop
  end if
  cores: do k = arg%l, arg%m
   if(associated(arg%u(k)%p)) deallocate(arg%u(k)%p)
   allocate(arg%u(k)%p(arg%r(k-1), arg%n(k), arg%r(k)), stat=ierr)
   if(ierr /= 0) then
    write(*,*) 'TT allocate fail: no memory'; stop
   end if
  end do cores
 end subroutine

 subroutine dtt_dealloc(arg)
  ! free the host cores and release the device engine that holds the resident train
  use ttx_c, only: ttx_destroy
  type(dtt),intent(inout) :: arg
  integer :: k
  do k = 1, tt_size
   if(associated(arg%u(k)%p)) then
    deallocate(arg%u(k)%p); nullify(arg%u(k)%p)
   end if
  end do
  if(c_associated(arg%ttx)) then
   call ttx_destroy(arg%ttx)
   arg%ttx = c_null_ptr
  end if
 end subroutine

 subroutine dtt_ones(arg)
  ! rank-one train of ones
  type(dtt),intent(inout) :: arg
  integer :: k
  if(arg%m < arg%l) return
  call dtt_release(arg)
  arg%r(arg%l-1:arg%m) = 1
  call dtt_alloc(arg)
  do k = arg%l, arg%m
   arg%u(k)%p(:,:,:) = 1.d0
  end do
 end subroutine

 subroutine dtt_pull(arg)
  ! refresh arg%r and arg%u from the device-resident tensor train
  use ttx_c
  type(dtt),intent(inout) :: arg
  integer(c_int32_t) :: rk(0:tt_size)
  integer :: k
  call ttx_check(ttx_get_ranks(arg%ttx,rk),'tt_lib')
  arg%r(0:arg%m)=rk(0:arg%m)
  call dtt_alloc(arg)
  do k=1,arg%m; call ttx_check(ttx_get_core(arg%ttx,int(k,c_int),arg%u(k)%p),'tt_lib'); end do
 end subroutine
 subroutine dtt_stage(arg,h,temp,who)
  ! device handle for a utility call: the resident train of arg (after dtt_dmrgg / read / ort / svd), else a temporary
  ! upload of the host cores -- trains built on the host (ones, =, +, *) carry no handle and are staged per call,
  ! so editing arg%u(k)%p between calls is always seen
  use ttx_c
  type(dtt),intent(in) :: arg
  type(c_ptr),intent(out) :: h
  logical,intent(out) :: temp
  character(len=*),intent(in) :: who
  integer(c_int32_t) :: nn(tt_size),rr(0:tt_size)
  double precision,allocatable :: x(:)
  integer :: k,sz,pos
  temp=.false.; h=arg%ttx
  if(c_associated(h))return
  if(arg%l.ne.1 .or. arg%m.lt.2)then;write(*,*)who,': the device engine holds trains with l=1, m>=2; got l,m: ',arg%l,arg%m;stop;endif
  if(.not.dtt_ready(arg))then;write(*,*)who,': tensor train is not allocated';stop;endif
  sz=0; do k=1,arg%m; sz=sz+arg%r(k-1)*arg%n(k)*arg%r(k); end do
  allocate(x(sz)); pos=0
  do k=1,arg%m
   x(pos+1:pos+size(arg%u(k)%p))=reshape(arg%u(k)%p,[size(arg%u(k)%p)]); pos=pos+size(arg%u(k)%p)
  end do
  nn(1:arg%m)=arg%n(1:arg%m); rr(0:arg%m)=arg%r(0:arg%m)
  call ttx_check(ttx_from_tt(h,int(arg%m,c_int32_t),nn,rr,x,0_c_int32_t),who)
  temp=.true.
 end subroutine
 subroutine dtt_ort(arg)
  use ttx_c
  type(dtt),intent(inout),target :: arg
  type(c_ptr) :: h
  logical :: temp
  call dtt_stage(arg,h,temp,'dtt_ort'); call ttx_check(ttx_ort(h),'dtt_ort')
  arg%ttx=h; call dtt_pull(arg)
  if(temp)then; call ttx_destroy(h); arg%ttx=c_null_ptr; endif
 end subroutine
 subroutine dtt_svd(arg,tol,rmax)
  use ttx_c
  type(dtt),intent(inout),target :: arg
  double precision,intent(in) :: tol
  integer,intent(in),optional :: rmax
  integer(c_int32_t) :: rm
  type(c_ptr) :: h
  logical :: temp
  rm=0; if(present(rmax))rm=rmax
  call dtt_stage(arg,h,temp,'dtt_svd'); call ttx_check(ttx_svd(h,tol,rm),'dtt_svd')
  arg%ttx=h; call dtt_pull(arg)
  if(temp)then; call ttx_destroy(h); arg%ttx=c_null_ptr; endif
 end subroutine
 double precision function dtt_norm(arg,tol) result(nrm)
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in),optional :: tol
  real(c_double) :: t
  type(c_ptr) :: h
  logical :: temp
  t=-1.d0; if(present(tol))t=tol
  call dtt_stage(arg,h,temp,'dtt_norm'); call ttx_check(ttx_norm(h,t,nrm),'dtt_norm')
  if(temp)call ttx_destroy(h)
 end function
 double precision function dtt_lognrm(arg,tol) result(nrm)
  ! lib/tt.f90:1114: log10 of the Frobenius norm as d log10 of the equalised core norm (finite beyond the double range)
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in),optional :: tol
  real(c_double) :: t
  type(c_ptr) :: h
  logical :: temp
  t=-1.d0; if(present(tol))t=tol
  call dtt_stage(arg,h,temp,'dtt_lognrm'); call ttx_check(ttx_lognrm(h,t,nrm),'dtt_lognrm')
  if(temp)call ttx_destroy(h)
 end function
 double precision function dtt_dot(x,y) result(dot)
  use ttx_c
  type(dtt),intent(in) :: x,y
  type(c_ptr) :: hx,hy
  logical :: tx,ty
  call dtt_stage(x,hx,tx,'dtt_dot'); call dtt_stage(y,hy,ty,'dtt_dot'); call ttx_check(ttx_dot(hx,hy,dot),'dtt_dot')
  if(tx)call ttx_destroy(hx)
  if(ty)call ttx_destroy(hy)
 end function
 function dtt_ijk_many(arg,ind) result(a)
  ! tijk at many multi-indices, ind(d,npts): one batched call on the device (ttx_ijk_batch, the engine chooses the path); a host
  ! train is staged for the call like for norm / dot_product; trains the engine does not hold (l /= 1, one core) go point by point
  use ttx_c
  type(dtt),intent(in) :: arg
  integer,intent(in) :: ind(:,:)
  double precision :: a(size(ind,2))
  integer(c_int32_t),allocatable :: ix(:,:)
  type(c_ptr) :: h
  logical :: temp
  integer :: p
  if(size(ind,2).eq.0)return
  if(.not.c_associated(arg%ttx) .and. (arg%l.ne.1 .or. arg%m.lt.2))then
   do p=1,size(ind,2); a(p)=dtt_ijk(arg,ind(:,p)); end do
   return
  end if
  allocate(ix(arg%m,size(ind,2))); ix=ind(1:arg%m,:)
  call dtt_stage(arg,h,temp,'dtt_ijk')
  call ttx_check(ttx_ijk_batch(h,int(size(ind,2),c_int64_t),ix,a,2_c_int32_t),'dtt_ijk')
  if(temp)call ttx_destroy(h)
  deallocate(ix)
 end function
 subroutine dtt_weights(arg,w,ww)
  ! the rank-1 train w (as the quad argument of dtt_quad) as d blocks of n(k) weights
  type(dtt),intent(in) :: arg,w
  real(c_double),allocatable,intent(out) :: ww(:)
  integer :: k,off
  allocate(ww(sum(arg%n(1:arg%m)))); off=0
  do k=1,arg%m; ww(off+1:off+arg%n(k))=w%u(k)%p(1,1:arg%n(k),1); off=off+arg%n(k); end do
 end subroutine
 subroutine dtt_contract(arg,keep,res,w)
  ! res = arg with every mode k where keep(k) = 0 summed against the weights w%u(k)%p(1,:,1) (w absent: plain sums); at least two
  ! modes are kept.  One call on the device (ttx_contract); a host train is staged for the call like for norm / dot_product.
  ! res holds the new train on the device and, pulled, in res%u.
  use ttx_c
  type(dtt),intent(in) :: arg
  integer,intent(in) :: keep(:)
  type(dtt),intent(inout) :: res
  type(dtt),intent(in),optional :: w
  integer(c_int32_t) :: kp(tt_size)
  real(c_double),allocatable,target :: ww(:)
  type(c_ptr) :: h,hn,wp
  logical :: temp
  integer :: k
  call dtt_dealloc(res)
  kp(1:arg%m)=keep(1:arg%m)
  wp=c_null_ptr
  if(present(w))then; call dtt_weights(arg,w,ww); wp=c_loc(ww); endif
  call dtt_stage(arg,h,temp,'dtt_contract')
  hn=c_null_ptr
  call ttx_check(ttx_contract(h,kp,wp,hn),'dtt_contract')
  if(temp)call ttx_destroy(h)
  res%l=1; res%m=0
  do k=1,arg%m
   if(keep(k).ne.0)then; res%m=res%m+1; res%n(res%m)=arg%n(k); endif
  end do
  res%ttx=hn; call dtt_pull(res)
 end subroutine
 subroutine dtt_modeapply(arg,m,a,res,mode)
  ! res = arg with a matrix applied to every mode k where m(k) > 0: res(.., j, ..) = sum_i A_k(j,i) arg(.., i, ..), mode k gets m(k)
  ! indices, the ranks stay; m(k) = 0 leaves mode k alone.  a holds the blocks A_k(m(k),n(k)) of the applied modes one after the
  ! other in mode order, each as Fortran stores an array a(m,n).  mode: 0 the sums over ascending i with a separate multiply and
  ! add, 1 the fp64 matrix cores, 2 (the default) the engine chooses.  One call on the device (ttx_mode_apply); a host train is
  ! staged for the call like for norm / dot_product.  res holds the new train on the device and, pulled, in res%u.
  use ttx_c
  type(dtt),intent(in) :: arg
  integer,intent(in) :: m(:)
  double precision,intent(in) :: a(*)
  type(dtt),intent(inout) :: res
  integer,intent(in),optional :: mode
  integer(c_int32_t) :: mm(tt_size),md
  type(c_ptr) :: h,hn
  logical :: temp
  integer :: k
  call dtt_dealloc(res)
  mm(1:arg%m)=m(1:arg%m)
  md=2; if(present(mode))md=mode
  call dtt_stage(arg,h,temp,'dtt_modeapply')
  hn=c_null_ptr
  call ttx_check(ttx_mode_apply(h,mm,a,md,hn),'dtt_modeapply')
  if(temp)call ttx_destroy(h)
  res%l=1; res%m=arg%m
  do k=1,arg%m
   res%n(k)=arg%n(k); if(m(k).gt.0)res%n(k)=m(k)
  end do
  res%ttx=hn; call dtt_pull(res)
 end subroutine
 subroutine dtt_basisval(arg,x,kind,a,b,res,mode,halve)
  ! res(p) = sum_i arg(i) prod_k phi_(i_k)(x(k,p)): the train in one function basis on all modes at the real points x(m,npts).
  ! kind 1: phi_j(t) = cos(j pi (t-a)/(b-a)), j = 0..n(k)-1, the first term halved where halve is present and true (a train of
  ! COS-method coefficients gives its density); kind 2: hat functions on n(k) equidistant nodes a + (b-a)(j-1)/(n(k)-1) (a train
  ! of grid values gives its piecewise-linear interpolant, constant outside [a,b]).  mode: 0 the definition's operation order, 1 the
  ! fp64 matrix cores, 2 (the default) the engine chooses.  One call on the device (ttx_basis_batch); a host train is staged for
  ! the call like for norm / dot_product.
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: x(:,:)
  integer,intent(in) :: kind
  double precision,intent(in) :: a,b
  double precision,intent(out) :: res(:)
  integer,intent(in),optional :: mode
  logical,intent(in),optional :: halve
  type(ttx_basis_t) :: bs(tt_size)
  real(c_double),allocatable,target :: nodes(:,:)
  real(c_double),allocatable :: xx(:,:)
  integer(c_int32_t) :: md
  type(c_ptr) :: h
  logical :: temp
  integer :: k,j
  if(size(x,2).eq.0)return
  md=2; if(present(mode))md=mode
  allocate(nodes(maxval(arg%n(1:arg%m)),arg%m),xx(arg%m,size(x,2))); xx=x(1:arg%m,:)
  do k=1,arg%m
   bs(k)%kind=kind; bs(k)%flags=0; bs(k)%a=a; bs(k)%b=b; bs(k)%nodes=c_null_ptr
   if(present(halve))then; if(halve)bs(k)%flags=TTX_BASIS_HALVE_FIRST; endif
   if(kind.eq.TTX_BASIS_LINEAR)then
    do j=1,arg%n(k); nodes(j,k)=a+(b-a)*dble(j-1)/dble(max(arg%n(k)-1,1)); end do
    bs(k)%nodes=c_loc(nodes(1,k))
   end if
  end do
  call dtt_stage(arg,h,temp,'dtt_basisval')
  call ttx_check(ttx_basis_batch(h,int(size(x,2),c_int64_t),xx,bs,res,md),'dtt_basisval')
  if(temp)call ttx_destroy(h)
  deallocate(nodes,xx)
 end subroutine
 subroutine dtt_marginals(arg,marg,w)
  ! marg(i,k), i = 1..n(k): arg summed over every mode but k against the weights (w absent: plain sums); marg has at least
  ! maxval(n) rows and m columns, entries beyond n(k) are set to zero.  One call on the device (ttx_marginals).
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(out) :: marg(:,:)
  type(dtt),intent(in),optional :: w
  real(c_double),allocatable,target :: ww(:)
  real(c_double),allocatable :: o(:)
  type(c_ptr) :: h,wp
  logical :: temp
  integer :: k,off
  wp=c_null_ptr
  if(present(w))then; call dtt_weights(arg,w,ww); wp=c_loc(ww); endif
  allocate(o(sum(arg%n(1:arg%m))))
  call dtt_stage(arg,h,temp,'dtt_marginals')
  call ttx_check(ttx_marginals(h,wp,o),'dtt_marginals')
  if(temp)call ttx_destroy(h)
  marg=0.d0; off=0
  do k=1,arg%m; marg(1:arg%n(k),k)=o(off+1:off+arg%n(k)); off=off+arg%n(k); end do
 end subroutine
 subroutine dtt_sample(arg,u,ind,w,fixed,logq,val)
  ! ind(:,p) = a multi-index drawn from arg with the uniforms u(:,p) by sequential conditional sampling, the last mode first
  ! (include/ttx.h: ttx_sample): for a train and weights without sign changes the indices follow |arg(i)| w(i) / Z.  w: rank-1
  ! weights as the quad argument of dtt_quad (absent: ones); fixed(k) = 0 draws mode k, f holds it at index f (absent: all drawn);
  ! logq(p) = log of the probability of ind(:,p), val(p) = arg at ind(:,p).  A failed sample has ind(:,p) = 0, logq NaN, val 0.
  ! One call on the device; a host train is staged for the call like for norm / dot_product.
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: u(:,:)
  integer,intent(out) :: ind(:,:)
  type(dtt),intent(in),optional :: w
  integer,intent(in),optional :: fixed(:)
  double precision,intent(out),target,optional :: logq(:),val(:)
  real(c_double),allocatable,target :: ww(:)
  real(c_double),allocatable :: uu(:,:)
  integer(c_int32_t),allocatable :: ix(:,:)
  integer(c_int32_t),target :: fx(tt_size)
  type(c_ptr) :: h,wp,fp,lp,vp
  logical :: temp
  integer :: npts
  npts=size(u,2)
  if(npts.eq.0)return
  wp=c_null_ptr; fp=c_null_ptr; lp=c_null_ptr; vp=c_null_ptr
  if(present(w))then; call dtt_weights(arg,w,ww); wp=c_loc(ww); endif
  if(present(fixed))then; fx(1:arg%m)=fixed(1:arg%m); fp=c_loc(fx); endif
  if(present(logq))lp=c_loc(logq)
  if(present(val))vp=c_loc(val)
  allocate(uu(arg%m,npts),ix(arg%m,npts)); uu=u(1:arg%m,1:npts)
  call dtt_stage(arg,h,temp,'dtt_sample')
  call ttx_check(ttx_sample(h,int(npts,c_int64_t),uu,wp,fp,ix,lp,vp),'dtt_sample')
  if(temp)call ttx_destroy(h)
  ind(1:arg%m,1:npts)=ix
  deallocate(uu,ix)
 end subroutine
 subroutine dtt_sample_sq(arg,u,ind,w,fixed,gamma,mode,logq,val)
  ! ind(:,p) = a multi-index drawn from the SQUARE of arg with the uniforms u(:,p), the squared-density sampler (include/ttx.h:
  ! ttx_sample_sq): for any train, signed or not, the indices follow (arg(i)^2 + gamma) w(i) / (Z + gamma prod W).  arg is meant to
  ! approximate the square root of a density.  w, fixed, logq, val as for sample, the weights non-negative; gamma >= 0 the defensive
  ! term (absent: 0); mode 0 = exact, 1 = MFMA, 2 = auto (absent: auto).  val(p) = arg at ind(:,p), not its square.
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: u(:,:)
  integer,intent(out) :: ind(:,:)
  type(dtt),intent(in),optional :: w
  integer,intent(in),optional :: fixed(:),mode
  double precision,intent(in),optional :: gamma
  double precision,intent(out),target,optional :: logq(:),val(:)
  real(c_double),allocatable,target :: ww(:)
  real(c_double),allocatable :: uu(:,:)
  integer(c_int32_t),allocatable :: ix(:,:)
  integer(c_int32_t),target :: fx(tt_size)
  type(c_ptr) :: h,wp,fp,lp,vp
  real(c_double) :: gm
  logical :: temp
  integer :: npts,md
  npts=size(u,2)
  if(npts.eq.0)return
  wp=c_null_ptr; fp=c_null_ptr; lp=c_null_ptr; vp=c_null_ptr
  gm=0.d0; if(present(gamma))gm=gamma
  md=2; if(present(mode))md=mode
  if(present(w))then; call dtt_weights(arg,w,ww); wp=c_loc(ww); endif
  if(present(fixed))then; fx(1:arg%m)=fixed(1:arg%m); fp=c_loc(fx); endif
  if(present(logq))lp=c_loc(logq)
  if(present(val))vp=c_loc(val)
  allocate(uu(arg%m,npts),ix(arg%m,npts)); uu=u(1:arg%m,1:npts)
  call dtt_stage(arg,h,temp,'dtt_sample_sq')
  call ttx_check(ttx_sample_sq(h,int(npts,c_int64_t),uu,wp,fp,gm,int(md,c_int32_t),ix,lp,vp),'dtt_sample_sq')
  if(temp)call ttx_destroy(h)
  ind(1:arg%m,1:npts)=ix
  deallocate(uu,ix)
 end subroutine
 subroutine dtt_sample_real(arg,u,nodes,x,cond,cell,logq,val)
  ! x(:,p) = a real point drawn with the uniforms u(:,p) from the piecewise-linear interpolant of the grid values arg on the nodes
  ! nodes(1:n(k),k), strictly ascending, by the inverse Rosenblatt transform, the last mode first (include/ttx.h: ttx_sample_real):
  ! for a train without sign changes the points follow the interpolant / Z.  cond(k): a NaN draws mode k, a number holds it at that
  ! coordinate (absent: all drawn); cell(k,p) = the cell of a drawn mode, 0 for a held one; logq(p) = log of the proposal's density at
  ! x(:,p); val(p) = the interpolant there (basisval with kind 2 on the same nodes).  A failed sample has x(:,p) NaN, cell 0, logq NaN,
  ! val 0.  With no samples (size(u,2) = 0) nothing is called and no output is touched.  One call on the device; a host train is
  ! staged for the call like for norm / dot_product.
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: u(:,:)
  double precision,intent(in) :: nodes(:,:)
  double precision,intent(out) :: x(:,:)
  double precision,intent(in),optional :: cond(:)
  integer,intent(out),optional :: cell(:,:)
  double precision,intent(out),target,optional :: logq(:),val(:)
  real(c_double),allocatable,target :: tt(:,:)
  real(c_double),allocatable :: uu(:,:),xx(:,:)
  integer(c_int32_t),allocatable,target :: cx(:,:)
  real(c_double),target :: cc(tt_size)
  type(c_ptr) :: h,cp,ip,lp,vp,rows(tt_size)
  logical :: temp
  integer :: npts,k
  npts=size(u,2)
  if(npts.eq.0)return
  cp=c_null_ptr; ip=c_null_ptr; lp=c_null_ptr; vp=c_null_ptr
  if(present(cond))then; cc(1:arg%m)=cond(1:arg%m); cp=c_loc(cc); endif
  if(present(logq))lp=c_loc(logq)
  if(present(val))vp=c_loc(val)
  allocate(uu(arg%m,npts),xx(arg%m,npts),tt(maxval(arg%n(1:arg%m)),arg%m)); uu=u(1:arg%m,1:npts)
  if(present(cell))then; allocate(cx(arg%m,npts)); ip=c_loc(cx); endif
  do k=1,arg%m; tt(1:arg%n(k),k)=nodes(1:arg%n(k),k); rows(k)=c_loc(tt(1,k)); end do
  call dtt_stage(arg,h,temp,'dtt_sample_real')
  call ttx_check(ttx_sample_real(h,int(npts,c_int64_t),uu,rows,cp,xx,ip,lp,vp),'dtt_sample_real')
  if(temp)call ttx_destroy(h)
  x(1:arg%m,1:npts)=xx
  if(present(cell))then; cell(1:arg%m,1:npts)=cx; deallocate(cx); endif
  deallocate(uu,xx,tt)
 end subroutine
 subroutine dtt_sample_sq_real(arg,u,nodes,x,cond,gamma,mode,cell,logq,val)
  ! x(:,p) = a real point drawn with the uniforms u(:,p) from the SQUARE of the piecewise-multilinear interpolant g of the grid values
  ! arg on the nodes nodes(1:n(k),k), the squared-density sampler on a continuous domain (include/ttx.h: ttx_sample_sq_real): for any
  ! train, signed or not, the points follow (g(x)^2 + gamma) / (Z + gamma V).  arg is meant to approximate the square root of a
  ! density.  cond, cell, logq, val as for sample_real; gamma >= 0 the defensive term (absent: 0); mode 0 = exact, 1 = MFMA, 2 = auto
  ! (absent: auto).  val(p) = g at x(:,p), not its square.  A host train is staged for the call like for norm / dot_product.
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: u(:,:)
  double precision,intent(in) :: nodes(:,:)
  double precision,intent(out) :: x(:,:)
  double precision,intent(in),optional :: cond(:),gamma
  integer,intent(in),optional :: mode
  integer,intent(out),optional :: cell(:,:)
  double precision,intent(out),target,optional :: logq(:),val(:)
  real(c_double),allocatable,target :: tt(:,:)
  real(c_double),allocatable :: uu(:,:),xx(:,:)
  integer(c_int32_t),allocatable,target :: cx(:,:)
  real(c_double),target :: cc(tt_size)
  type(c_ptr) :: h,cp,ip,lp,vp,rows(tt_size)
  real(c_double) :: gm
  logical :: temp
  integer :: npts,k,md
  npts=size(u,2)
  if(npts.eq.0)return
  cp=c_null_ptr; ip=c_null_ptr; lp=c_null_ptr; vp=c_null_ptr
  gm=0.d0; if(present(gamma))gm=gamma
  md=2; if(present(mode))md=mode
  if(present(cond))then; cc(1:arg%m)=cond(1:arg%m); cp=c_loc(cc); endif
  if(present(logq))lp=c_loc(logq)
  if(present(val))vp=c_loc(val)
  allocate(uu(arg%m,npts),xx(arg%m,npts),tt(maxval(arg%n(1:arg%m)),arg%m)); uu=u(1:arg%m,1:npts)
  if(present(cell))then; allocate(cx(arg%m,npts)); ip=c_loc(cx); endif
  do k=1,arg%m; tt(1:arg%n(k),k)=nodes(1:arg%n(k),k); rows(k)=c_loc(tt(1,k)); end do
  call dtt_stage(arg,h,temp,'dtt_sample_sq_real')
  call ttx_check(ttx_sample_sq_real(h,int(npts,c_int64_t),uu,rows,cp,gm,int(md,c_int32_t),xx,ip,lp,vp),'dtt_sample_sq_real')
  if(temp)call ttx_destroy(h)
  x(1:arg%m,1:npts)=xx
  if(present(cell))then; cell(1:arg%m,1:npts)=cx; deallocate(cx); endif
  deallocate(uu,xx,tt)
 end subroutine
 subroutine dtt_rosenblatt_sq_real(arg,x,nodes,u,cond,gamma,mode,cell,logq,val)
  ! u(:,p) = the uniforms that sample_sq_real maps to the given point x(:,p): the forward Rosenblatt map of the squared interpolant
  ! (include/ttx.h: ttx_rosenblatt_sq_real), with logq(p) the log of the proposal's density (g(x)^2 + gamma) / (Z + gamma V) at the
  ! point and val(p) = g there.  nodes, cond, gamma, mode as for sample_sq_real.  u is 0 and cell 0 on a held mode; a point with a
  ! drawn coordinate outside the nodes' range has a column of NaN in u.  A host train is staged for the call like for norm / dot_product.
  use ttx_c
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: x(:,:)
  double precision,intent(in) :: nodes(:,:)
  double precision,intent(out) :: u(:,:)
  double precision,intent(in),optional :: cond(:),gamma
  integer,intent(in),optional :: mode
  integer,intent(out),optional :: cell(:,:)
  double precision,intent(out),target,optional :: logq(:),val(:)
  real(c_double),allocatable,target :: tt(:,:)
  real(c_double),allocatable :: uu(:,:),xx(:,:)
  integer(c_int32_t),allocatable,target :: cx(:,:)
  real(c_double),target :: cc(tt_size)
  type(c_ptr) :: h,cp,ip,lp,vp,rows(tt_size)
  real(c_double) :: gm
  logical :: temp
  integer :: npts,k,md
  npts=size(x,2)
  if(npts.eq.0)return
  cp=c_null_ptr; ip=c_null_ptr; lp=c_null_ptr; vp=c_null_ptr
  gm=0.d0; if(present(gamma))gm=gamma
  md=2; if(present(mode))md=mode
  if(present(cond))then; cc(1:arg%m)=cond(1:arg%m); cp=c_loc(cc); endif
  if(present(logq))lp=c_loc(logq)
  if(present(val))vp=c_loc(val)
  allocate(uu(arg%m,npts),xx(arg%m,npts),tt(maxval(arg%n(1:arg%m)),arg%m)); xx=x(1:arg%m,1:npts)
  if(present(cell))then; allocate(cx(arg%m,npts)); ip=c_loc(cx); endif
  do k=1,arg%m; tt(1:arg%n(k),k)=nodes(1:arg%n(k),k); rows(k)=c_loc(tt(1,k)); end do
  call dtt_stage(arg,h,temp,'dtt_rosenblatt_sq_real')
  call ttx_check(ttx_rosenblatt_sq_real(h,int(npts,c_int64_t),xx,rows,cp,gm,int(md,c_int32_t),uu,ip,lp,vp),'dtt_rosenblatt_sq_real')
  if(temp)call ttx_destroy(h)
  u(1:arg%m,1:npts)=uu
  if(present(cell))then; cell(1:arg%m,1:npts)=cx; deallocate(cx); endif
  deallocate(uu,xx,tt)
 end subroutine
 subroutine dtt_topk(arg,k,ind,val,bound,which,fixed,mode,nfound)
  ! the k largest elements of arg by a beam search on the device (include/ttx.h: ttx_topk): ind(:,j) and val(j), j = 1 .. nfound,
  ! ordered by which (0: |val| descending, the default; 1: val descending; 2: val ascending), rows beyond nfound zero.  Every
  ! element that is not returned has |arg(i)| <= bound up to rounding (NaN if a score was NaN): bound <= |val(nfound)| under
  ! which = 0 proves the rows, bound <= |val(1)| the maximum.  fixed(k) = 0 searches mode k, f holds it at index f (absent: all
  ! searched); mode: 0 plain loops, 1 matrix cores, 2 the engine chooses (the default).  A host train is staged for the call.
  use ttx_c
  type(dtt),intent(in) :: arg
  integer,intent(in) :: k
  integer,intent(out) :: ind(:,:)
  double precision,intent(out) :: val(:),bound
  integer,intent(in),optional :: which,fixed(:),mode
  integer,intent(out),optional :: nfound
  integer(c_int32_t),allocatable :: ix(:,:)
  real(c_double),allocatable :: vv(:)
  integer(c_int32_t),target :: fx(tt_size)
  integer(c_int32_t) :: nf,wh,md
  real(c_double) :: bd
  type(c_ptr) :: h,fp
  logical :: temp
  wh=0; md=2; fp=c_null_ptr
  if(present(which))wh=which
  if(present(mode))md=mode
  if(present(fixed))then; fx(1:arg%m)=fixed(1:arg%m); fp=c_loc(fx); endif
  allocate(ix(arg%m,max(k,1)),vv(max(k,1)))
  call dtt_stage(arg,h,temp,'dtt_topk')
  call ttx_check(ttx_topk(h,int(k,c_int32_t),wh,fp,md,nf,ix,vv,bd),'dtt_topk')
  if(temp)call ttx_destroy(h)
  ind(1:arg%m,1:k)=ix(:,1:k); val(1:k)=vv(1:k); bound=bd
  if(present(nfound))nfound=nf
  deallocate(ix,vv)
 end subroutine
 double precision function dtt_ijk(arg,ind) result(a)
  ! lib/tt.f90:630-652: one element; a resident train is asked on the device, a host train is contracted here
  use ttx_c
  type(dtt),intent(in) :: arg
  integer,intent(in) :: ind(:)
  integer(c_int32_t) :: ix(arg%m)
  double precision :: b(1)
  if(c_associated(arg%ttx))then
   ix=ind(1:arg%m)
   call ttx_check(ttx_ijk(arg%ttx,ix,a),'dtt_ijk')
  else
   if(arg%r(arg%l-1).ne.1 .or. arg%r(arg%m).ne.1)then; a=-4.d0; return; endif
   if(any(ind(1:arg%m-arg%l+1).le.0).or.any(ind(1:arg%m-arg%l+1).gt.arg%n(arg%l:arg%m)))then; a=-3.d0; return; endif
   call dtt_elem(arg,ind,b); a=b(1)
  end if
 end function

 ! ---- host-side generics (lib/tt.f90): plain Fortran on the host cores ----------------------------------
 logical function dtt_ready(arg) result(l)
  ! lib/tt.f90:1306: dimensions set and every core allocated with the right shape
  type(dtt),intent(in) :: arg
  integer :: k
  l=.false.
  if(arg%l.gt.arg%m)return
  do k=arg%l,arg%m
   if(arg%n(k).le.0 .or. arg%r(k-1).le.0 .or. arg%r(k).le.0)return
   if(.not.associated(arg%u(k)%p))return
   if(any(shape(arg%u(k)%p).ne.[arg%r(k-1),arg%n(k),arg%r(k)]))return
  end do
  l=.true.
 end function
 subroutine dtt_release(arg)
  ! drop the device train of arg (it is about to receive new contents)
  use ttx_c, only: ttx_destroy
  type(dtt),intent(inout) :: arg
  if(c_associated(arg%ttx))then; call ttx_destroy(arg%ttx); arg%ttx=c_null_ptr; endif
 end subroutine
 subroutine dtt_assign(b,a)
  ! lib/tt.f90:1012-1020: b = a is a DEEP copy of the cores.  The device train stays with a: b is a host train (its own
  ! storage, no handle), so dealloc(a) and dealloc(b) each release only what they own (the one exception, below: a is the
  ! result of axpby / hadamard, which nobody else can release)
  type(dtt),intent(inout) :: b
  type(dtt),intent(in) :: a
  integer :: k
  call dtt_release(b)
  b%l=a%l; b%m=a%m; b%n(a%l:a%m)=a%n(a%l:a%m); b%r(a%l-1:a%m)=a%r(a%l-1:a%m)
  call dtt_alloc(b)
  do k=a%l,a%m; b%u(k)%p=a%u(k)%p; end do
  ! the result of axpby / hadamard hands its device train to the variable it is assigned to
  if(c_associated(a%ttx))then
   if(c_associated(a%ttx,tt_pending))then; b%ttx=a%ttx; tt_pending=c_null_ptr; endif
  end if
 end subroutine
 subroutine ztt_assign(b,a)
  ! lib/tt.f90:1021-1032
  type(ztt),intent(inout) :: b
  type(ztt),intent(in) :: a
  integer :: k
  b%l=a%l; b%m=a%m; b%n(a%l:a%m)=a%n(a%l:a%m); b%r(a%l-1:a%m)=a%r(a%l-1:a%m)
  call ztt_alloc(b)
  do k=a%l,a%m; b%u(k)%p=a%u(k)%p; end do
  b%ttx=a%ttx                        ! borrowed from the dtt it was made from, never released by a ztt
 end subroutine
 subroutine dtt_copy(a,b,low)
  ! lib/tt.f90:1047-1058: copy a into b with the first core placed at index low (default b%l)
  type(dtt),intent(in) :: a
  type(dtt),intent(inout) :: b
  integer,intent(in),optional :: low
  integer :: k,ll,mm
  ll=b%l; if(present(low))ll=low
  mm=ll-a%l+a%m
  call dtt_release(b)
  b%l=ll; b%m=mm; b%n(ll:mm)=a%n(a%l:a%m); b%r(ll-1:mm)=a%r(a%l-1:a%m)
  if(.not.all(a%n(a%l:a%m)>0))return
  if(.not.all(a%r(a%l-1:a%m)>0))return
  call dtt_alloc(b)
  do k=a%l,a%m; b%u(ll-a%l+k)%p=a%u(k)%p; end do
 end subroutine
 subroutine dtt_zeros(arg)
  ! lib/tt.f90:1375: rank-one train of zeros
  type(dtt),intent(inout) :: arg
  integer :: k
  if(arg%m < arg%l) return
  call dtt_release(arg)
  arg%r(arg%l-1:arg%m)=1
  call dtt_alloc(arg)
  do k=arg%l,arg%m; arg%u(k)%p=0.d0; end do
 end subroutine
 double precision function dtt_numel(arg) result(s)
  ! lib/tt.f90:817: number of entries of the full tensor
  type(dtt),intent(in) :: arg
  integer :: k
  s=0.d0; if(arg%l.gt.arg%m)return
  s=1.d0; do k=arg%l,arg%m; s=s*arg%n(k); end do
 end function
 integer function dtt_mem(arg) result(sz)
  ! lib/tt.f90:1266: numbers stored in the cores
  type(dtt),intent(in) :: arg
  integer :: k
  sz=0; do k=arg%l,arg%m; sz=sz+arg%r(k-1)*arg%n(k)*arg%r(k); end do
 end function
 subroutine dtt_say(arg)
  ! lib/tt.f90:1200: short description on stdout
  type(dtt),intent(in) :: arg
  write(*,'(a,i2,a,i4,a,f6.2,a,i12)') 'dtt[',arg%l,':',arg%m,']: rank ',dtt_rank(arg),' memory ',dtt_mem(arg)
  write(*,'(a,1x,64i4)') 'n: ',arg%n(arg%l:min(arg%m,arg%l+63))
  write(*,'(a,64i4)') 'r: ',arg%r(arg%l-1:min(arg%m,arg%l+62))
 end subroutine
 subroutine dtt_elem(arg,ind,a)
  ! lib/tt.f90:678-700: the r(l-1) x r(m) block of the train at a multi-index, left to right
  type(dtt),intent(in) :: arg
  integer,intent(in) :: ind(:)
  double precision,intent(out) :: a(*)
  double precision,allocatable :: x(:,:),z(:,:)
  integer :: k,l,m
  l=arg%l; m=arg%m
  if(any(ind(1:m-l+1).le.0).or.any(ind(1:m-l+1).gt.arg%n(l:m)))then;write(*,*)'dtt_elem: wrong index: ',ind;stop;endif
  allocate(x(arg%r(l-1),arg%r(l))); x=arg%u(l)%p(:,ind(1),:)
  do k=l+1,m
   allocate(z(arg%r(l-1),arg%r(k))); z=matmul(x,arg%u(k)%p(:,ind(k-l+1),:))
   call move_alloc(z,x)
  end do
  a(1:arg%r(l-1)*arg%r(m))=reshape(x,[arg%r(l-1)*arg%r(m)])
 end subroutine
 double precision function dtt_value(arg,x) result(val)
  ! lib/tt.f90:702-731: the train read as a function on [0,1]^dd, each coordinate spread over (m-l+1)/dd modes
  ! (most significant digit in the LAST mode of its block)
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: x(:)
  integer :: dd,per,id,j,pos,i,ind(tt_size)
  double precision :: xx
  ind=0; val=0.d0; dd=size(x)
  if(arg%l.gt.arg%m)return
  per=(arg%m-arg%l+1)/dd
  do id=1,dd
   xx=x(id)
   if(xx.lt.0.d0)return
   if(xx.gt.1.d0)xx=xx-int(xx)
   do j=1,per
    pos=arg%l+(id-1)*per+per-j
    i=int(arg%n(pos)*xx); if(i.eq.arg%n(pos))i=arg%n(pos)-1
    ind(pos-arg%l+1)=i+1
    xx=xx*arg%n(pos)-i
   end do
  end do
  val=dtt_ijk(arg,ind(1:arg%m-arg%l+1))
 end function
 double precision function dtt_value0(arg,x) result(val)
  type(dtt),intent(in) :: arg
  double precision,intent(in) :: x
  val=dtt_value(arg,[x])
 end function
 double precision function dtt_sumall(arg) result(val)
  ! lib/tt.f90:770-790: sum of all entries = product of the mode-summed cores, left to right
  type(dtt),intent(in) :: arg
  double precision,allocatable :: x(:,:),z(:,:)
  integer :: k,l,m
  l=arg%l; m=arg%m; val=0.d0
  if(arg%r(l-1).gt.1 .or. arg%r(m).gt.1)then; val=-1.d0; return; endif
  allocate(x(arg%r(l-1),arg%r(l))); x=sum(arg%u(l)%p,dim=2)
  do k=l+1,m
   allocate(z(arg%r(l-1),arg%r(k))); z=matmul(x,sum(arg%u(k)%p,dim=2))
   call move_alloc(z,x)
  end do
  val=x(1,1)
 end function
 function dtt_plus_dtt(a,b) result(c)
  ! lib/tt.f90:928-946: c = a + b, ranks add, cores become block diagonal (first core: side by side, last: stacked)
  type(dtt),intent(in) :: a,b
  type(dtt) :: c
  integer :: k,l,m,ra0,ra1
  if(.not.(dtt_ready(a).and.dtt_ready(b)))return
  l=a%l; m=a%m
  c%l=l; c%m=m; c%n=a%n; c%r=0; c%r(l-1)=a%r(l-1); c%r(m)=a%r(m); c%r(l:m-1)=a%r(l:m-1)+b%r(l:m-1)
  call dtt_alloc(c)
  do k=l,m
   c%u(k)%p=0.d0
   ra0=a%r(k-1); ra1=a%r(k)
   if(k.eq.l)then
    c%u(k)%p(:,:,1:ra1)=a%u(k)%p; if(m.gt.l)c%u(k)%p(:,:,ra1+1:)=b%u(k)%p
   else if(k.eq.m)then
    c%u(k)%p(1:ra0,:,:)=a%u(k)%p; c%u(k)%p(ra0+1:,:,:)=b%u(k)%p
   else
    c%u(k)%p(1:ra0,:,1:ra1)=a%u(k)%p; c%u(k)%p(ra0+1:,:,ra1+1:)=b%u(k)%p
   end if
  end do
 end function
 function dtt_plus_d(a,b) result(c)
  ! lib/tt.f90:966-986: c = a + b*ones
  type(dtt),intent(in) :: a
  double precision,intent(in) :: b
  type(dtt) :: c,e
  integer :: k
  if(.not.dtt_ready(a))return
  e%l=a%l; e%m=a%m; e%n=a%n; call dtt_ones(e); e%u(e%l)%p=b
  c=dtt_plus_dtt(a,e)
  do k=e%l,e%m; deallocate(e%u(k)%p); end do
 end function
 function dtt_mul_dt(a,b) result(c)
  ! lib/tt.f90:989-998: c = a*b, the scalar goes into the first core
  double precision,intent(in) :: a
  type(dtt),intent(in) :: b
  type(dtt) :: c
  integer :: k
  c%l=b%l; c%m=b%m; c%n=b%n; c%r=b%r; call dtt_alloc(c)
  do k=b%l,b%m; c%u(k)%p=b%u(k)%p; end do
  c%u(b%l)%p=a*c%u(b%l)%p
 end function
 double precision function dtt_rank(arg) result(er)
  ! effective rank: the r for which a train with all inner ranks r stores as many numbers as arg does,
  ! i.e. the positive root of  a r^2 + b r - S = 0,  S = sum r(k-1) n(k) r(k)
  type(dtt),intent(in) :: arg
  integer :: k,first,last,ncores,inner,edge
  double precision :: stored
  first = arg%l; last = arg%m; ncores = last-first+1
  er = -1.d0
  if(ncores <= 0) return
  er = 0.d0
  if(ncores == 1) return
  stored = 0.d0
  do k = first, last
   stored = stored + arg%r(k-1)*arg%n(k)*arg%r(k)
  end do
  er = stored
  if(stored == 0.d0) return
  edge = arg%r(first-1)*arg%n(first) + arg%n(last)*arg%r(last)
  if(ncores == 2) then
   er = stored/edge
   return
  end if
  inner = sum(arg%n(first+1:last-1))
  er = (dsqrt(edge*edge + 4.d0*inner*stored) - edge)/(2.d0*inner)
 end function
end module
