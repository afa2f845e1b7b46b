! coefficients_mod -- drop-in for the fork's lib/coefficients.f90: the multivariate COS coefficients of a correlated Gaussian,
!   calc_coefficient(d, ind, n) = 2 (1/(b-a))^d  sum over the sign vectors s of  Re( exp(-i a sum t) phi(t) ),
!   t_j = pi s_j (ind_j - 1) / (b - a),
! with mu, Sigma, a, b set by init_coefficients and the sign vectors of s_vector_mod.  This is the host form of the function; handed
! to dtt_dmrgg it is recognised (identify_coscoeff below) and the sweep evaluates the device integrand TTX_FUN_COSCOEFF instead.
module coefficients_mod
 use s_vector_mod
 use funcs
 use constants
 use ttx_c,only:TTX_FUN_HOST,TTX_FUN_COSCOEFF
 use iso_c_binding,only:c_double
 use dmrgg_lib,only:coscoeff_identify
 implicit none
 private :: identify_coscoeff
 double precision,allocatable :: coeff_mu(:)
 double precision,allocatable :: coeff_sigma(:,:)
 double precision :: lower_bound,upper_bound
contains
 subroutine init_coefficients(n_dimensions,mean,cov,lower,upper)
  integer,intent(in) :: n_dimensions
  double precision,intent(in) :: mean(n_dimensions),cov(n_dimensions,n_dimensions),lower,upper
  if(.not.allocated(coeff_mu))allocate(coeff_mu(n_dimensions))
  if(.not.allocated(coeff_sigma))allocate(coeff_sigma(n_dimensions,n_dimensions))
  coeff_mu=mean
  coeff_sigma=cov
  lower_bound=lower
  upper_bound=upper
  coscoeff_identify=>identify_coscoeff      ! dtt_dmrgg may now recognise calc_coefficient (dmrgg_lib: identify_nopar)
 end subroutine

 double precision function calc_coefficient(n_dimensions,ind,mode_sizes) result(f)
  integer,intent(in) :: n_dimensions,ind(n_dimensions),mode_sizes(n_dimensions)
  double precision :: t(n_dimensions),ob,acc
  complex*16 :: e
  integer :: k,j
  ob=1/(upper_bound-lower_bound)
  acc=0.d0
  do k=1,size(s_vectors,2)
   do j=1,n_dimensions
    t(j)=((pi*dble(s_vectors(j,k)))*dble(ind(j)-1))*ob
   end do
   e=exp(dcmplx(0.d0,-1.d0)*lower_bound*sum(t))
   acc=acc+real(e*gaussian_chf_nd(n_dimensions,t,coeff_mu,coeff_sigma))
  end do
  f=2.d0*ob**n_dimensions*acc
 end function
 subroutine identify_coscoeff(fun,m,n,fid,aux)
  ! `fun` called without par: is it the fork's calc_coefficient (coefficients_mod)?  Only when coefficients_mod holds mu and Sigma
  ! for m dimensions and s_vectors is exactly the generated set of m dimensions (TTX_INTEGRAND=coscoeff requires the same) is `fun`
  ! compared with the COS-coefficient formula at NPROBE small multi-indices (their values are far from cancellation).  Fail
  ! closed, as identify: every probe must agree to 1e-12 of the sum of |terms| and at least three must lie far above that noise;
  ! anything else runs through the host callback.  TTX_INTEGRAND=host forces the callback.
  double precision,external :: fun
  integer,intent(in) :: m,n(*)
  integer,intent(out) :: fid
  real(c_double),allocatable,intent(out) :: aux(:)
  integer,parameter :: NPROBE=6
  integer :: ind(m),t,i,k,j,stat,good
  double precision :: f,g,mag,ob,tt(m),q,dm,st,e
  logical :: ready,ok
  character(len=32) :: env
  fid=TTX_FUN_HOST
  call get_environment_variable('TTX_INTEGRAND',env,status=stat)
  if(stat.ne.0)env='auto'
  if(trim(env).eq.'host')return
  ready=m.le.20 .and. allocated(coeff_mu) .and. allocated(coeff_sigma) .and. allocated(s_vectors)
  if(ready)ready=size(coeff_mu).eq.m .and. all(shape(coeff_sigma).eq.[m,m]) .and. all(shape(s_vectors).eq.[m,2**(m-1)])
  if(ready)then
   do k=1,2**(m-1)
    do j=1,m
     if(s_vectors(j,k).ne.merge(-1,1,j.gt.1 .and. btest(k-1,max(j-2,0))))ready=.false.
    end do
   end do
  end if
  if(trim(env).eq.'coscoeff')then
   if(.not.ready)then;write(*,*)'dtt_dmrgg: TTX_INTEGRAND=coscoeff needs init_coefficients and generate_s_vectors for ',m,' dimensions';stop;endif
  else if(trim(env).ne.'auto')then
   return                                              ! ising / stdnorm / mvn need par: not this function
  else
   if(.not.ready)return
   ob=1/(upper_bound-lower_bound); good=0
   do t=1,NPROBE
    do i=1,m
     ind(i)=min(n(i),1+mod(i*t+t/2,3))
    end do
    if(t.eq.1)ind=1
    f=fun(m,ind,n)
    g=0.d0; mag=0.d0
    do k=1,2**(m-1)                                    ! the formula, sign vectors generated here
     do j=1,m
      tt(j)=merge(-1.d0,1.d0,j.gt.1 .and. btest(k-1,max(j-2,0)))*pi*dble(ind(j)-1)*ob
     end do
     dm=sum(tt*coeff_mu); q=sum(matmul(coeff_sigma,tt)*tt); st=sum(tt)
     e=exp(-0.5d0*q)
     g=g+e*(cos(lower_bound*st)*cos(dm)+sin(lower_bound*st)*sin(dm)); mag=mag+e
    end do
    g=2.d0*ob**m*g; mag=2.d0*ob**m*mag
    ok=abs(f-g).le.1d-12*mag
    if(.not.ok)return
    if(abs(g).gt.1d-6*mag .and. mag.gt.1d-250)good=good+1
   end do
   if(good.lt.3)return
  end if
  fid=TTX_FUN_COSCOEFF
  allocate(aux(m+m*m+2))
  aux(1:m)=coeff_mu; aux(m+1:m+m*m)=reshape(coeff_sigma,[m*m]); aux(m+m*m+1)=lower_bound; aux(m+m*m+2)=upper_bound
 end subroutine
end module coefficients_mod
