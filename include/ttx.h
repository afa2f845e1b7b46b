/*
 * ttx.h -- C-ABI of libttx.so, the MI355X-native engine for the reference's dtt_dmrgg greedy-cross sweep.
 *
 * The reference (aukeschaap/ttcross) has no FFI layer: its boundary for this path is the Fortran module
 * interface of lib/dmrgg.f90 / lib/tt.f90 that the test_crs_* drivers `use`.  Each entry point below names
 * the reference interface it replaces; INTEGRATION.md shows the ISO_C_BINDING stubs with which the
 * reference's own modules (or the drop-in modules in ttcross_amd/fortran/) bind to them.
 *
 * Plain C types only (no torch / HIP types); every function returns 0 on success, a TTX_E* code
 * otherwise, and ttx_last_error() gives the message (the Fortran shim turns it into the reference's
 * `write(*,*) ...; stop`).  One host thread per engine handle.  The engine NEVER falls back to the CPU:
 * without a gfx950 device ttx_create fails with TTX_ENODEV.
 */
#ifndef TTX_H
#define TTX_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TTX_OK 0
#define TTX_EINVAL 1   /* bad argument (reference: print + stop, e.g. lib/dmrgg.f90:88-91,114-117,590-592) */
#define TTX_ENODEV 2   /* no usable HIP device                                                           */
#define TTX_EHIP 3     /* HIP / RCCL runtime error                                                       */
#define TTX_ESTATE 4   /* call out of order                                                              */

/* integrands.  The drivers' integrands are built in (device code) and selected by id; a user `fun` of the
 * reference (lib/dmrgg.f90:18) runs either on the host through a callback (TTX_FUN_HOST) or on the GPU, written as a HIP
 * __device__ function against include/ttx_device_fun.h and loaded as a code object (TTX_FUN_DEVICE). */
#define TTX_FUN_ISING 1    /* dfunc_ising_discr, test_crs_ising.f90:176-218 (par(2n+1) = 1/2/3 -> C/D/E) */
#define TTX_FUN_STDNORM 2  /* integrand, test_crs_stdnorm.f90:154-170                                     */
#define TTX_FUN_MVN 3      /* integrand -> mvn_pdf, test_crs_mvn.f90:156-172, lib/mvn_pdf.f90:63-83       */
#define TTX_FUN_HOST 4     /* any user `fun` (lib/dmrgg.f90:18), evaluated on the HOST: ttx_set_integrand_host */
/* calc_coefficient, the fork's COS coefficients (test_crs_coscoeff.f90, lib/coefficients.f90): evaluated on the device
 * (ttx_coscoeff.h).  aux = [mu(1:d), Sigma(1:d,1:d) column-major, a, b], naux = d + d*d + 2; par unused.  ttx_create refuses
 * (TTX_EINVAL) a wrong naux, non-finite aux, a >= b, d > 20, and problems whose bound on |t'mu| or |a sum t| over the index
 * box exceeds the range of the integrand's own sin / cos (2^19).  Mode sizes may differ.  TTX_ARITH=fast leaves it exact. */
#define TTX_FUN_COSCOEFF 5
#define TTX_FUN_DEVICE 6   /* any user `fun`, evaluated on the DEVICE by a code object the caller supplies: ttx_set_integrand_device */
#define TTX_FUN_TRAINS 7   /* fun(i) = g(x_1(i), ..., x_m(i)), x_t resident trains on the engine's device: ttx_set_integrand_trains */
#define TTX_FUN_PULLBACK 8 /* fun(i) = h(x, logq, val), the grid point of i pulled back through resident squared-train transports: ttx_set_integrand_pullback */

#define TTX_ARITH_EXACT 0
#define TTX_ARITH_FAST 1

typedef struct ttx_engine ttx_engine;

/* Arguments of dtt_dmrgg(arg, fun, par, accuracy, maxrank, mybonds, pivoting, neval, quad, tru),
 * lib/dmrgg.f90:11-26.  arg%l is always 1 (as in every driver); arg%m = d; arg%n = n[]. */
typedef struct ttx_config {
    int32_t d;              /* arg%m : number of TT cores                                            */
    const int32_t *n;       /* arg%n(1:d) : mode sizes                                               */
    int32_t fun_id;         /* TTX_FUN_* : replaces the `fun` callback                               */
    const double *par;      /* par(*) as the driver builds it (nodes, weights, id)                   */
    int32_t npar;
    const double *aux;      /* TTX_FUN_MVN: mu[d], inv_cov[d*d] column-major, det (mvn_data)         */
    int32_t naux;
    const double *quadw;    /* quad : rank-1 TT of per-mode weights, d blocks of n[k]; NULL = absent */
    double accuracy;        /* < 0 : absent                                                          */
    int32_t maxrank;        /* required (>= 1): also sizes device storage                            */
    int32_t pivoting;       /* -1 full, 0 lottery only, p >= 1 rook (reference default 3)            */
    double tru;             /* tru (only used for the `err` column)                                  */
    int32_t has_tru;
    int32_t nproc;          /* total number of bond groups ("MPI ranks" of the reference), >= 1, < d */
    const int32_t *mybonds; /* own(0:nproc), 1-based bonds; NULL -> share(1, d-1) lib/default.f90:78 */
    int32_t device;         /* HIP device ordinal                                                    */
    int32_t world_rank;     /* this process within the multi-GPU job (0 when single process)         */
    int32_t world_size;     /* number of processes (GPUs); groups are split contiguously over them   */
    int32_t verbose;        /* 1: print the reference's per-sweep log lines (lib/dmrgg.f90:971-1008) */
    int32_t arith;          /* TTX_ARITH_EXACT (0, default): every fp64 operation of the integrand in the reference's order,
                             * results bit-identical to the reference restatement; TTX_ARITH_FAST (1): products / sums of the
                             * O(d^2) integrands (Ising D/E, mvn) re-associated, O(d) per fiber element, results equal to
                             * rounding (tolerance-checked).  The environment variable TTX_ARITH=fast|exact overrides 0.     */
} ttx_config;

/* one line of the reference's per-sweep report (lib/dmrgg.f90:971-1008) */
typedef struct ttx_sweep_rec {
    int32_t it;
    int32_t dir;            /* 0 '::', 1 '>>', 2 '<<' */
    double erank;
    int64_t neval;
    double val;
    double amax, pivotmax, pivotmin;
    double seconds;         /* since the start of ttx_run */
} ttx_sweep_rec;

const char *ttx_last_error(void);
int ttx_version(void);   /* 2: loadable device integrands; 3: ttx_ijk_batch, ttx_ijk_batch_dev, ttx_value_batch (ttx_contract,
                          * ttx_marginals, ttx_lincomb, ttx_hadamard, ttx_algebra_last and ttx_mode_apply came later without a new number:
                          * look the symbols up) */

/* allocate device state for one dtt_dmrgg problem (replaces the implicit set-up of lib/dmrgg.f90:58-148) */
int ttx_create(ttx_engine **out, const ttx_config *cfg);
void ttx_destroy(ttx_engine *h);

/* RCCL bootstrap for world_size > 1 (replaces mpi_init / MPI_COMM_WORLD, test_crs_ising.f90:31-36):
 * rank 0 calls ttx_comm_unique_id, the host layer broadcasts the 128 bytes, every rank calls ttx_comm_init. */
int ttx_comm_unique_id(uint8_t id[128]);
int ttx_comm_init(ttx_engine *h, const uint8_t id[128]);

/* Alternative transport for world_size > 1 when RCCL cannot be used (and for multi-process tests on one GPU):
 * the host layer supplies MPI-like primitives on HOST buffers; the engine stages messages through pinned memory.
 * sendrecv: send ns bytes to rank `to` (skip if to < 0) and receive nr bytes from rank `from` (skip if < 0);
 * allreduce: in place on `count` doubles, op 0 = sum, 1 = max.  Both return 0 on success. */
typedef struct ttx_transport {
    void *ctx;
    int (*sendrecv)(void *ctx, int to, const void *sbuf, int64_t ns, int from, void *rbuf, int64_t nr);
    int (*allreduce)(void *ctx, double *buf, int64_t count, int op);
} ttx_transport;
int ttx_set_transport(ttx_engine *h, const ttx_transport *t);
/* Built-in host transport for processes of ONE node, over a POSIX shared-memory segment `name` (every rank passes the same
 * name; rank 0 creates it): the same two primitives, no MPI and no RCCL needed.  Used by the Fortran drop-in layer
 * (TTX_TRANSPORT=shm) and by tests that run several engine processes on one GPU, where RCCL cannot. */
int ttx_comm_init_shm(ttx_engine *h, const char *name);

/* The reference's integrand callback, `double precision,external :: fun` called as fun(m, ind, n, par) (lib/dmrgg.f90:18,
 * walked by dmrgg_fun :1053-1078): Fortran calling convention, everything by reference; ind and n are default integers.
 * An engine created with fun_id = TTX_FUN_HOST evaluates every fiber through this function on the host -- each
 * evaluating kernel first hands the multi-indices it needs to the host, the host calls `fun` from a pool of threads
 * (TTX_HOST_THREADS, else OMP_NUM_THREADS, else the hardware; `fun` must be thread-safe, as under the reference's
 * OpenMP loops), and the kernel continues with the values.  par is passed through untouched (may be NULL: the
 * reference's `par` is optional).  The sweep logic, pivot search and factor updates stay on the device; results are
 * those of the reference for the same `fun`.  With pivoting = -1 the superblock goes to the host one column (k,q) at a time. */
typedef double (*ttx_host_fun)(const int32_t *m, const int32_t *ind, const int32_t *n, const double *par);
/* LIFETIME: the engine keeps the two pointers, it does not copy par.  They must stay valid for every later call that evaluates
 * (ttx_run, ttx_accchk); a caller whose par may move or die calls ttx_set_integrand_host again before such a call (the
 * Fortran dtt_accchk does, with the fun / par it was given: lib/dmrgg.f90:1081 checks against ITS arguments). */
int ttx_set_integrand_host(ttx_engine *h, ttx_host_fun fun, const double *par);
int64_t ttx_host_calls(const ttx_engine *h);                      /* calls of `fun` made by the last ttx_run */

/* The user's `fun` on the DEVICE, for an engine created with fun_id = TTX_FUN_DEVICE (ttx_config.par / npar are not used by it).
 * The integrand is a __device__ function turned into kernels by TTX_DEVICE_INTEGRAND(name) / TTX_DEVICE_INTEGRAND_WAVE(name) of
 * include/ttx_device_fun.h and compiled with `hipcc --genco --offload-arch=gfx950 -O3 -ffp-contract=off`.  The sweep is the one
 * of TTX_FUN_HOST -- every evaluating kernel runs in two passes -- but between the passes the integrand's slot kernel runs on the
 * engine's stream: no value crosses to the host, ttx_host_calls stays 0, nothing is synchronised.
 *   image, nbytes : the code object in memory, whatever hipModuleLoadData accepts (a gfx950 ELF or the offload bundle hipcc
 *                   --genco writes); the engine keeps its own copy
 *   name          : the integrand's name as given to the header macro (one code object may hold several)
 *   par(1:npar)   : the caller's parameter array.  UNLIKE ttx_set_integrand_host, which keeps the caller's pointer, the engine
 *                   COPIES par to the device here: later changes of the caller's array are not seen (set the integrand again)
 * TTX_ESTATE: engine not created with TTX_FUN_DEVICE.  TTX_EINVAL: null / empty image, unreadable file, bytes that are no code
 * object, a code object the runtime refuses (e.g. built for another GPU), no integrand `name` in it, an integrand compiled against
 * another TTX_DEVFUN_ABI, more than 64 KB of LDS per workgroup, npar < 0 or par missing.  After a refusal the engine is as before.
 * Setting an integrand again replaces the first and unloads its module; ttx_destroy unloads it and frees the par copy; a replica
 * (ttx_replicate, ttx_accchk on a multi-process engine) shares both.  ttx_run / ttx_accchk before an integrand is set: TTX_ESTATE. */
int ttx_set_integrand_device(ttx_engine *h, const void *image, int64_t nbytes, const char *name, const double *par, int32_t npar);
int ttx_set_integrand_device_file(ttx_engine *h, const char *path, const char *name, const double *par, int32_t npar);
/* the loaded integrand at npts multi-indices (ind row-major, 1-based; out of range: TTX_EINVAL), through the code object's list
 * kernel: check that a device function computes what its author thinks before a sweep depends on it.  An engine created with
 * TTX_FUN_TRAINS is served too: the m operands at the listed indices, then the combiner. */
int ttx_eval_device(ttx_engine *h, int64_t npts, const int32_t *ind /* [npts][d] */, double *out /* [npts] */);

/* Cross approximation of a FUNCTION OF RESIDENT TRAINS, fun(i) = g(x_1(i), ..., x_m(i)), for an engine created with fun_id =
 * TTX_FUN_TRAINS (ttx_config.par / npar are not used; d <= 2048; one process, any number of bond groups): squares and products whose
 * Hadamard ranks pass 128, quotients, roots, products of three and more trains, without a core leaving the device (TT-Toolbox:
 * multifuncrs).  The sweep is the one of TTX_FUN_DEVICE; between the two passes of every evaluating kernel one kernel (k_tf_slots,
 * ttcross_amd/csrc/ttx_trainfun.h) evaluates every operand at the requested multi-indices, one wave per element, in the operation
 * sequence of ttx_ijk_batch's TTX_EVAL_EXACT, and applies the combiner: the value of operand t is ttx_ijk_batch(x[t], ind,
 * TTX_EVAL_EXACT) bit for bit, and a run equals, bit for bit, a TTX_FUN_HOST run whose callback walks the same cores in that order.
 * The built-in combiners are plain IEEE operations in the order written here; TTX_ARITH=fast leaves the integrand exact.
 *   m, x  : 1 <= m <= TTX_TRAINS_MAX engines that hold a train on the engine's device, with the engine's mode sizes n(1:d) and ranks
 *           up to 128; the same engine may appear several times (x * x).  The engine records the HANDLES.  At the start of every
 *           ttx_run, ttx_accchk and ttx_eval_device it looks at the operands again and rebuilds their device blocks (core pointers,
 *           ranks) in its own work space: an operand that was ttx_ort-ed or ttx_svd-ed in between is seen with its new ranks, and
 *           an operand stays free for calls of its own between runs.
 *           LIFETIME: the caller keeps every operand alive, and leaves it unchanged, while such a call is running, and does not
 *           destroy an operand before the engine (or sets other operands first).
 *   image, nbytes / path, name, par, npar : a loaded combiner, TTX_DEVICE_COMBINER(name) of include/ttx_device_fun.h, with the
 *           conventions and refusals of ttx_set_integrand_device (par is COPIED to the device)
 * TTX_ESTATE: engine not created with TTX_FUN_TRAINS; an operand without a train.  TTX_EINVAL: m outside 1..TTX_TRAINS_MAX, an op
 * that does not fit m, a null operand, an operand spread over processes (as ttx_ijk refuses it), on another device, with other mode
 * sizes, or the engine itself; every message names the operand.  After a refusal the engine is as before.  Setting again replaces
 * the operands and the combiner; a replica (ttx_replicate) shares them.  ttx_run / ttx_accchk / ttx_eval_device before a
 * successful set, and ttx_comm_init / ttx_comm_init_shm / ttx_set_transport on such an engine: TTX_ESTATE.
 * ttx_trainfun_last: of the last ttx_run or ttx_eval_device, the launches of the slot (list) kernel, the elements it evaluated and,
 * with ttx_set_profile on, its milliseconds (HIP events; 0 otherwise).  Any pointer may be NULL.
 * Added without a new ttx_version: look the symbols up. */
#define TTX_TRAINS_MAX 8
#define TTX_TOP_PRODUCT 1     /* p = v[0]; p = p * v[t], t = 1 .. m-1 (1 <= m <= TTX_TRAINS_MAX) */
#define TTX_TOP_RATIO   2     /* v[0] / v[1]           (m == 2)                                  */
#define TTX_TOP_SQRTABS 3     /* sqrt(fabs(v[0]))      (m == 1)                                  */
#define TTX_TOP_DEVICE  4     /* a loaded combiner: ttx_set_integrand_trains_device              */
int ttx_set_integrand_trains(ttx_engine *h, int32_t m, ttx_engine *const *x, int32_t op);
int ttx_set_integrand_trains_device(ttx_engine *h, int32_t m, ttx_engine *const *x, const void *image, int64_t nbytes,
                                    const char *name, const double *par, int32_t npar);
int ttx_set_integrand_trains_device_file(ttx_engine *h, int32_t m, ttx_engine *const *x, const char *path,
                                         const char *name, const double *par, int32_t npar);
int ttx_trainfun_last(const ttx_engine *h, double *ms, int64_t *launches, int64_t *elements);

/* Cross approximation of a device function PULLED BACK THROUGH RESIDENT SQUARED-TRAIN TRANSPORTS, for an engine created with fun_id =
 * TTX_FUN_PULLBACK (ttx_config.par / npar are not used; d <= 2048; one process, any number of bond groups): the next layer of a
 * layered (deep inverse Rosenblatt) transport, built without a point leaving the device.  The engine's grid is a reference grid in
 * [0,1]^d: for a multi-index i, u^(m)_k = ref_k[i_k - 1].  Then, for t = m, m-1, .., 1, as a sequence of operations,
 *     (x^(t), lq_t, val_t) = ttx_sample_sq_real(layer[t-1].x, u = u^(t), layer[t-1].nodes, cond = NULL, layer[t-1].gamma, TTX_EVAL_EXACT)
 *     u^(t-1) = x^(t)
 * and the results are x = x^(1); logq = lq_m, then logq = logq + lq_t for t = m-1 .. 1; val = val_1.  Layer 1 is the outermost layer,
 * the one built first: its nodes span the physical box.  A sample that fails at any layer gives the sampler's failed row -- x NaN,
 * logq NaN, val 0.0 -- and is counted in nfailed.  x, logq and val are, bit for bit, what that chain of public calls returns.
 * The integrand's value is what the loaded function returns: a TTX_DEVICE_COMBINER(name) of include/ttx_device_fun.h, called with
 * m = d + 2 and v = [x_1 .. x_d, logq, val].  The sweep is the one of TTX_FUN_TRAINS: between the two passes of every evaluating
 * kernel one kernel (k_pb_slots, ttcross_amd/csrc/ttx_pullback.h) transports the requested points, one wave per element, and the
 * combiner's slot kernel runs behind it; ttx_host_calls stays 0, nothing is synchronised.
 *   m, layer : 1 <= m <= TTX_PULLBACK_MAX layers.  layer[t].x holds a train on the engine's device with d modes of at least two
 *           indices each (all modes are drawn) and ranks up to 128; layer[t].nodes[k] are the n_k(x) finite, strictly ascending nodes
 *           of its mode k, for t >= 1 (layers 2 and up) from exactly 0.0 to exactly 1.0, because the layer's output is the next
 *           layer's uniforms; layer[t].gamma >= 0 is its defensive term.  The same engine may appear as several layers, with the same
 *           nodes and gamma (both layers read one head; other nodes or gamma for one engine are refused).  The node rows are COPIED,
 *           the engine HANDLES are recorded: at the start of every ttx_run, ttx_accchk, ttx_eval_device and ttx_pullback_points the
 *           engine looks at the layers again (a layer that was ttx_ort-ed or ttx_svd-ed in between is seen with its new ranks), runs
 *           the sampler's head pass on each distinct layer engine and waits for it once.
 *           LIFETIME: as for ttx_set_integrand_trains; in addition the caller makes no call on a layer's engine while a run of this
 *           engine is in flight: the layer's head tables live in the layer's own work space.
 *   ref   : ref[k] are the n_k(h) entries of the reference grid of mode k, each in [0, 1] (COPIED)
 *   image, nbytes / path, name, par, npar : the combiner, with the conventions and refusals of ttx_set_integrand_trains_device.
 *           image == NULL (path == NULL) records the layers only: ttx_pullback_points works, ttx_run, ttx_accchk and ttx_eval_device
 *           answer TTX_ESTATE.
 * ttx_pullback_points: x, logq, val at npts multi-indices (ind row-major, 1-based; out of range: TTX_EINVAL); logq, val may be NULL.
 * ttx_eval_device on such an engine: the combiner's value at the listed indices.
 * TTX_ESTATE: engine not created with TTX_FUN_PULLBACK.  TTX_EINVAL, each before any launch and with the engine as before: m outside
 * 1..TTX_PULLBACK_MAX; a null layer or the engine itself; a layer without a train, spread over processes or on another device; with
 * another d; with a rank above 128; with a mode of one index; a node row that is missing, not finite or not strictly ascending, or
 * for t >= 2 does not run from 0.0 to 1.0; a ref row that is missing or has an entry outside [0, 1]; gamma negative or not finite;
 * the combiner's refusals; more LDS per wave (two states, two sheets of the largest layer mode, the point, the index row) than a
 * workgroup can have.  Every message names the layer and the mode.  Creation, ttx_comm_init*, ttx_set_transport, replicas: as for
 * TTX_FUN_TRAINS.  TTX_PB_GRID (environment) caps the grid of the transport kernels.
 * ttx_pullback_last: of the last ttx_run, ttx_eval_device or ttx_pullback_points, the launches of the transport kernel, the elements it
 * evaluated, the failed samples among them and, with ttx_set_profile on, its milliseconds with the combiner's (HIP events; 0
 * otherwise).  Any pointer may be NULL.  Added without a new ttx_version: look the symbols up. */
#define TTX_PULLBACK_MAX 8
typedef struct { ttx_engine *x; const double *const *nodes; double gamma; } ttx_layer;   /* nodes: [d] host rows of n_k(x) */
int ttx_set_integrand_pullback     (ttx_engine *h, int32_t m, const ttx_layer *layer, const double *const *ref /* [d] host rows of n_k(h) */,
                                    const void *image, int64_t nbytes, const char *name, const double *par, int32_t npar);
int ttx_set_integrand_pullback_file(ttx_engine *h, int32_t m, const ttx_layer *layer, const double *const *ref,
                                    const char *path, const char *name, const double *par, int32_t npar);
int ttx_pullback_points(ttx_engine *h, int64_t npts, const int32_t *ind /* [npts][d], 1-based */, double *x /* [npts][d] */, double *logq, double *val);
int ttx_pullback_last(const ttx_engine *h, double *ms, int64_t *launches, int64_t *elements, int64_t *nfailed);

/* dtt_dmrgg itself: initial cross, sweeps until maxrank / 3 strikes, finalisation dtt_lua (lib/dmrgg.f90:151-1049) */
int ttx_run(ttx_engine *h);

/* results */
int ttx_num_sweeps(const ttx_engine *h);                          /* records available (sweep 0 included) */
int ttx_get_sweeps(const ttx_engine *h, ttx_sweep_rec *out, int cap);
int ttx_get_tapes(const ttx_engine *h, int32_t *out /* [nsweeps-1][d+1][4] */, int64_t cap);
int64_t ttx_neval(const ttx_engine *h);                           /* `neval` of dtt_dmrgg                 */
double ttx_seconds(const ttx_engine *h);                          /* wall time of the last ttx_run        */
int ttx_get_ranks(const ttx_engine *h, int32_t *r /* [d+1] */);   /* arg%r(0:d)                           */
int64_t ttx_core_size(const ttx_engine *h, int k);                /* r(k-1)*n(k)*r(k) or 0 if not owned   */
int ttx_get_core(const ttx_engine *h, int k, double *buf);        /* arg%u(k)%p, column-major, k = 1..d   */

/* dtt_quad(arg, quad) on the finalised cores (lib/dmrgg.f90:1261-1415); w = d blocks of n[k] weights, NULL = sum */
int ttx_quad(ttx_engine *h, const double *w, double *val);

/* dtt_accchk(nlot, arg, einf, efro, ainf, afro, fun, par, pivot), lib/dmrgg.f90:1081-1166: nlot random samples of
 * |fun - TT| drawn from the run-time RNG stream where dtt_dmrgg left it (irnd, lib/rnd.f90:83-88); element
 * evaluation as dtt_ijk (lib/tt.f90:630-652).  As in the reference every rank needs all cores: on a multi-process engine the
 * call is COLLECTIVE and works on a replica of the job's train (ttx_replicate); every process gets the same numbers.
 * pivot: d ints (worst sample) or NULL. */
int ttx_accchk(ttx_engine *h, int32_t nlot, double *einf, double *efro, double *ainf, double *afro, int32_t *pivot);

/* tt_lib utilities on the tensor train resident on the device.  ttx_norm / ttx_dot / ttx_zquad / ttx_write on a
 * multi-process engine are COLLECTIVE (ztt_quad folds per-process partial products, lib/dmrgg.f90:1418-1523; the others work on a
 * replica, ttx_replicate); ttx_ort / ttx_svd / ttx_ijk change or address single cores and take single-process engines (or a replica).
 * ttx_ort  : dtt_ort  (lib/tt.f90:130-198)  left-to-right Householder QR, in place
 * ttx_svd  : dtt_svd  (lib/tt.f90:307-368)  rounding: ort, then truncated SVD right-to-left; tol relative (>= 0; a NaN or negative
 *            tol, or rmax < 0, is TTX_EINVAL; at tol >= 1 every rank stops at 1)
 *            (lib/mat.f90:433-458 chop), rmax <= 0: absent
 * ttx_norm : dtt_norm (lib/tt.f90:1074-1092) Frobenius norm, tol < 0: absent (the TT itself is left unchanged)
 * ttx_dot  : dtt_dot  (lib/tt.f90:1155-1175) scalar product of two resident TTs with equal mode sizes
 * ttx_ijk  : dtt_ijk  (lib/tt.f90:630-652)  one element, ind = d 1-based indices */
int ttx_ort(ttx_engine *h);
int ttx_svd(ttx_engine *h, double tol, int32_t rmax);
int ttx_norm(ttx_engine *h, double tol, double *val);
/* ttx_lognrm: dtt_lognrm (lib/tt.f90:1114-1132) log10 of the Frobenius norm, computed as d log10 of the norm of the core that carries
 * it after the norm equalisation (tol < 0: absent, as ttx_norm) -- finite for trains whose norm lies outside the double range */
int ttx_lognrm(ttx_engine *h, double tol, double *val);
int ttx_dot(ttx_engine *hx, ttx_engine *hy, double *val);
int ttx_ijk(ttx_engine *h, const int32_t *ind, double *val);
/* The train at a BATCH of multi-indices or coordinate vectors, evaluated on the device by kernels of their own (ttx_ijk above
 * costs about 2 d launches per element).  The engines ttx_ijk takes; a multi-process engine is refused as by ttx_ijk.  The train is
 * not modified and the work space is the engine's own (allocated on first use, freed by ttx_destroy); batches are processed in
 * chunks of TTX_IJK_CHUNK points (environment; default 2^18, 2^17 above maxrank 64), so memory stays bounded.
 *   mode : TTX_EVAL_EXACT  one wave per point, the operation sequence of dtt_ijk's matmul chain in index order (sums from 0 over
 *                          ascending k, separate multiply and add): bit-identical to the oracle's restatement
 *          TTX_EVAL_MFMA   per mode the points are sorted by their index and all points of one index multiply the same core slice
 *                          as a GEMM on the fp64 matrix cores: equal to EXACT to rounding (another summation order); a point's value
 *                          does not depend on the other points of the batch
 *          TTX_EVAL_AUTO   the engine chooses (ttx_eval_last_mode tells what ran)
 *   ind  : npts rows of d 1-based indices.  A point with an entry outside 1..n(k) gets -3.0 (lib/tt.f90:638); no core is read for it.
 *   The engine holds trains of at least two cores (ttx_create, ttx_from_tt): there is no resident train of one core to evaluate.
 *   npts = 0 succeeds and launches nothing; a null pointer with npts > 0, npts < 0 or an unknown mode: TTX_EINVAL.
 * ttx_ijk_batch_dev takes pointers on the engine's device (e.g. torch tensors), enqueues on the engine's stream and synchronises
 * before it returns: no index crosses the host link.
 * ttx_value_batch is dtt_value (lib/tt.f90:702-728) for npts coordinate vectors x(1:dd) (row-major): the index digits are formed on
 * the device as the reference forms them (mm = d / dd digits per coordinate, last mode of a group first, i = int(n xx), i = n
 * clamped to n - 1, xx = xx n - i; xx > 1 reduced by xx - int(xx)); a negative coordinate gives 0.0, modes left without a digit
 * give the -3.0 of dtt_ijk.  Coordinates must be below 2^31 (NaN included: TTX_EINVAL). */
#define TTX_EVAL_EXACT 0
#define TTX_EVAL_MFMA 1
#define TTX_EVAL_AUTO 2
int ttx_ijk_batch(ttx_engine *h, int64_t npts, const int32_t *ind /* [npts][d], 1-based */, double *out /* [npts] */, int32_t mode);
int ttx_ijk_batch_dev(ttx_engine *h, int64_t npts, const int32_t *ind_dev, double *out_dev, int32_t mode);
int ttx_value_batch(ttx_engine *h, int64_t npts, int32_t dd, const double *x /* [npts][dd] */, double *out, int32_t mode);
int ttx_eval_last_mode(const ttx_engine *h);       /* TTX_EVAL_EXACT or TTX_EVAL_MFMA: what the last batch ran with (-1: none yet) */
/* ztt_quad (lib/dmrgg.f90:1418-1523) of the (real) resident TT with COMPLEX rank-1 weights, batched over nf weight
 * sets (the 32 frequencies of test_crs_chf.f90:153-168 in one call): w = nf blocks of sum(n) interleaved (re, im)
 * doubles, out = nf (re, im) pairs.  Multi-process engines: collective, the value on every process. */
int ttx_zquad(ttx_engine *h, int32_t nf, const double *w, double *out);

/* Partial contraction of the resident train with rank-1 weights.
 *   keep : d entries, 1 = the mode survives, 0 = it is summed against its weights
 *   w    : d blocks of n[k] weights as for ttx_quad (blocks of kept modes are ignored); NULL = all ones (plain sums)
 *   *out : a new single-process engine without integrand (as ttx_from_tt: everything but ttx_run / ttx_accchk works),
 *          owned by the caller.  The source engine and its work space are not modified.
 * A slice is the same operation with a unit vector as the weight of the fixed mode.
 * The result: let the kept modes be k_1 < ... < k_m and M_k = sum_i w_k(i) G_k(:, i, :) for a contracted mode.  New core j is
 * P_j G_(k_j), P_j the ordered product of the M_k between k_(j-1) and k_j (none: no product is formed); the M_k after k_m are
 * multiplied into the last new core from the right.  Ranks: r'(0) = 1, r'(j) = r(k_j) for j < m, r'(m) = 1.  With nothing
 * contracted the result is a bit-identical deep copy.
 * Arithmetic is plain double, as ttx_quad: there is NO running exponent, a train whose partial products leave the double range
 * over- or underflows.  Weights are not inspected: NaN and Inf propagate.  Sums have a fixed order: a call repeats bit for bit.
 * Everything is enqueued on the source engine's stream and the call synchronises before it returns; the new cores are written
 * device to device into storage sized by the new train's own largest rank and mode: no core crosses the host link.
 * TTX_EINVAL: null keep / out, a keep entry other than 0 or 1, fewer than two kept modes (the engine holds trains of at least two
 * cores: ttx_marginals gives one-mode marginals, ttx_quad the full sum); TTX_ESTATE: an engine without a train; a multi-process
 * engine is refused as by ttx_ijk (a replica, ttx_replicate, is accepted).  After a refusal *out is NULL and nothing stays allocated. */
int ttx_contract(ttx_engine *h, const int32_t *keep, const double *w, ttx_engine **out);
/* all d one-mode marginals in one call: out = d blocks of n[k], block k(i) = sum over every other mode against its weights */
int ttx_marginals(ttx_engine *h, const double *w, double *out);
/* the mode-sum kernel of the last ttx_contract / ttx_marginals on this engine: its milliseconds (HIP events) and the bytes of the
 * cores it summed, 8 sum r(k-1) n(k) r(k) over the contracted modes (0 ms when nothing was contracted) */
int ttx_contract_modesum(const ttx_engine *h, double *ms, double *bytes);

/* Sums and elementwise products of resident trains, assembled on the device (ttcross_amd/csrc/ttx_algebra.h).  Every element of a
 * new core is a copy, a zero or ONE rounded product, so the results are predictable bit for bit.
 * ttx_lincomb : sum_t coef[t] x[t] for m >= 1 trains with equal d and mode sizes: dtt_plus_dtt for m terms composed with dtt_mul_dt
 *               (lib/tt.f90:928-946, 989-998).  Ranks r'(0) = r'(d) = 1, r'(k) = sum_t r_t(k) on interior bonds.  Core 1 is the
 *               terms' first cores side by side, each multiplied by its coef[t] (the only multiply, as the dscal of dtt_mul_dt);
 *               interior cores are block diagonal in term order with explicit 0.0 off the blocks; core d is the terms' last cores
 *               stacked.  The same engine may appear several times (x + x, x - x).  Coefficients are not inspected: 0, NaN and Inf
 *               act as the multiply makes them act.  m = 1 is a scaled deep copy.
 * ttx_hadamard: z(i) = x(i) y(i).  Ranks r'(k) = r_x(k) r_y(k); 0-based, core k is
 *               Z[ib rx0 + ia, j, kb rx1 + ka] = X[ia, j, ka] Y[ib, j, kb] -- the x index runs fastest on both bonds, one multiply
 *               per element.  x and y may be the same engine.
 * *out is a new single-process engine without integrand (as ttx_contract's), owned by the caller; the operands and their work
 * space are not modified.  Every new rank must be <= 128, the engine's cap: a larger sum or product is TTX_EINVAL with the bond
 * and the value in the message.  The cap is NOT lifted and nothing is rounded on the fly: round the operands (ttx_svd) first,
 * or the result afterwards.  A tile count above 2^31 - 1 is TTX_EINVAL.
 * Everything is enqueued on x[0]'s stream (x's for ttx_hadamard) and the call synchronises before it returns; the OTHER operands
 * must be idle -- under the rule of one host thread per engine, no call on them may be in flight in another thread.
 * TTX_EINVAL: null pointers, m < 1, unequal d or mode sizes, engines on different devices (all pointer and count checks come
 * before any device call); TTX_ESTATE: an engine without a train; a multi-process engine is refused as by ttx_ijk (a replica,
 * ttx_replicate, is accepted).  After a refusal *out is NULL and nothing stays allocated.
 * ttx_algebra_last, called with x[0] (x for ttx_hadamard): the assembly kernel of the last ttx_lincomb / ttx_hadamard on that
 * engine -- its milliseconds (HIP events), 8 x the source core elements it read, 8 x sum r'(k-1) n(k) r'(k) it wrote.
 * Added without a new ttx_version: look the symbols up. */
int ttx_lincomb(int32_t m, const double *coef /* [m] */, ttx_engine *const *x /* [m] */, ttx_engine **out);
int ttx_hadamard(ttx_engine *x, ttx_engine *y, ttx_engine **out);
int ttx_algebra_last(const ttx_engine *h, double *ms, double *bytes_read, double *bytes_written);

/* A rounded sum of resident trains, on the device (ttcross_amd/csrc/ttx_roundsum.h): sum_t coef[t] x[t] rounded by one randomized
 * right-to-left and one left-to-right pass ("randomize-then-orthogonalize", Al Daas et al., SIAM J. Sci. Comput. 2023), without
 * ever forming a core of rank sum_t r_t.  ttx_lincomb keeps its refusal; this is the call for sums beyond rank 128.
 * Inputs: m trains with equal d and mode sizes n_k on one device, ranks r_t(k), S(k) = sum_t r_t(k); coefficients; a sketch rank
 * L = rsketch (0 means 128); a seed.
 *  1. Sketch ranks, on the host: l(0) = l(d) = 1; l(k) = min(L, S(k), prod_{j<=k} n_j, prod_{j>k} n_j), a product no longer
 *     multiplied once it is above 128; then left to right l(k) <= l(k-1) n_k and right to left l(k-1) <= n_k l(k), so that every
 *     matrix that is QR-factored is tall or square.
 *  2. Sketch train Omega_k (l(k-1), n_k, l(k)), uniform on (-1, 1), generated on the device from (seed, k, x), x the flat
 *     column-major index a + l(k-1) (i + n_k b), k = 1 .. d, by uint64 arithmetic:
 *         z = seed + 0x9E3779B97F4A7C15 * ((k << 40) + x + 1)
 *         z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z = z ^ (z >> 31)
 *         value = (bit 63 of z ? -1 : +1) * ((z >> 11) & (2^52 - 1)) * 2^-52
 *  3. Right to left: W_t(d) = [1]; W_t(k-1) = sum_i X_{t,k}(:, i, :) W_t(k) Omega_k(:, i, :)^T.  The W_t(k) of all terms are
 *     stacked in term order; after each step the stack is multiplied by 2^-e, (f, e) = frexp(max |W|) (e = 0 for zeros or a stack
 *     that holds an Inf or a NaN) -- one power of two per bond for all terms: it changes no bit of any Q and keeps long trains in range.
 *  4. Left to right: Y_t(1) = coef[t] X_{t,1} (the only use of the coefficients, as in ttx_lincomb); the Y_t(k) side by side
 *     are Y(k) (l(k-1) n_k rows, S(k) columns).  For k = 1 .. d-1: Z = Y(k) W(k); Z = Q R by the engine's QR; new core k = Q;
 *     M = Q^T Y(k); Y_t(k+1) = M_t x_1 X_{t,k+1}.  New core d = sum_t Y_t(d) in term order.  Y is plain double without a running
 *     exponent, as in ttx_contract.
 *  5. tol >= 0: the truncation of ttx_svd(tol, rmax) runs on the new train; tol < 0 skips it and the result is the left-orthogonal
 *     train of step 4 with ranks l(k).
 *   mode : TTX_EVAL_MFMA runs steps 3 and the products of step 4 with the cores on v_mfma_f64_16x16x4_f64, TTX_EVAL_EXACT by plain
 *          loops (the checker), TTX_EVAL_AUTO lets the engine choose by the work of the call.  Summation orders are fixed: a call
 *          repeats bit for bit.  The two modes agree to rounding.
 * Limits: m <= 256; S(k) <= 4096 at every bond.  TTX_EINVAL, each before any device call: null pointers, m < 1, m > 256 (the message
 * names the value), rsketch outside 0 .. 128, rmax < 0, a NaN tol, an unknown mode, then the operand checks of ttx_lincomb, then a
 * rank sum above 4096 (the message names the bond and the value).  TTX_ESTATE and multi-process engines as for ttx_lincomb.
 * Everything is enqueued on x[0]'s stream, the other operands must be idle, and the call synchronises before it returns.  *out is
 * a new single-process engine without integrand whose storage is sized by max l(k); work space comes from x[0].  The operands are
 * not modified; the same engine may appear several times.  After a refusal *out is NULL and nothing stays allocated.
 * ttx_roundsum_last, called with x[0]: milliseconds (HIP events) of the right-to-left pass, of the GEMMs, of the QRs (with Q's way
 * into the new core and its transpose) and of the advance launches of the last call, summed over the steps (the three phases of the
 * second pass alternate d - 1 times, so they are timed by a chain of events that x[0] keeps and reuses, 4 d of them); flops = the products of
 * steps 3 and 4 (the QRs not counted); the sketch ranks l(0 .. d); the mode that ran (-1: none yet).  Any pointer may be NULL.
 * Added without a new ttx_version: look the symbols up. */
int ttx_lincomb_round(int32_t m, const double *coef, ttx_engine *const *x, int32_t rsketch, double tol, int32_t rmax,
                      uint64_t seed, int32_t mode, ttx_engine **out);
int ttx_roundsum_last(const ttx_engine *h, double *ms /* [4]: sketch, gemm, qr, advance */, double *flops, int32_t *lsk /* [d+1] */, int32_t *mode_ran);

/* Matrices applied to chosen modes of the resident train, on the device (ttcross_amd/csrc/ttx_modeapply.h): the n-mode product,
 * G'_k(a, j, b) = sum_i A_k(j, i) G_k(a, i, b) with A_k of m_k x n_k (TT-Toolbox: ttm).  COS coefficients to values on a grid,
 * regridding, cumulative sums and differentiation along a mode.  ttx_contract is the case m_k = 1 followed by dropping the mode.
 *   m    : d entries; 0 = mode k is left alone, m_k >= 1 = mode k gets m_k indices
 *   A    : the matrices of the applied modes only, concatenated in mode order; block k is m_k x n_k, column-major: A_k(j, i) lies at
 *          j + m_k i (a Fortran a(m, n) passes as it is).  Entries are not inspected: NaN and Inf propagate.
 *   mode : TTX_EVAL_EXACT  s = 0.0; for i = 0 .. n_k-1: s = s + A_k(j, i) * G_k(a, i, b) -- ascending i, separate multiply and add
 *          TTX_EVAL_MFMA   the same sums on the fp64 matrix cores, in the instruction's own order: equal to EXACT to rounding.  An
 *                          element does not depend on the tiling of other cores or on the grid; no atomics, no split of the sum
 *                          across workgroups: a call repeats bit for bit
 *          TTX_EVAL_AUTO   the engine chooses by the work of the call (ttx_mode_apply_last tells what ran)
 *   *out : a new single-process engine without integrand (as ttx_contract's), owned by the caller.  Ranks are unchanged, mode sizes
 *          are m_k where applied and n_k elsewhere, storage is sized by the new train's own largest mode.  A core that is not
 *          applied is a bit-identical device-to-device copy; with every m(k) = 0 the result is a bit-identical deep copy.  The
 *          source engine and its work space are not modified.
 * Everything is enqueued on the source engine's stream and the call synchronises before it returns; the matrices go to the device
 * once per call (ttx_mode_apply_dev reads them in place, on the engine's device); no core crosses the host link.
 * TTX_EINVAL, each before any device call: a null h, m or out; a null A while some m(k) > 0; a negative m(k); an unknown mode; a
 * new mode size the engine's limits refuse, m_k > 32000 or largest rank times m_k > 131072 (the message names the mode and the
 * value).  TTX_ESTATE: an engine without a train; a multi-process engine is refused as by ttx_ijk (a replica, ttx_replicate, is
 * accepted).  After a refusal *out is NULL and nothing stays allocated.
 * ttx_mode_apply_last: the apply launch of the last call on this engine -- its milliseconds (HIP events; 0 when no mode was
 * applied), bytes_read = 8 sum r0 n_k r1 over the applied modes plus the matrices, bytes_written = 8 sum r0 m_k r1, flops =
 * 2 sum r0 r1 n_k m_k, and the mode that ran (-1: none yet).  Any pointer may be NULL.
 * Added without a new ttx_version: look the symbols up. */
int ttx_mode_apply    (ttx_engine *h, const int32_t *m /* [d] */, const double *A, int32_t mode, ttx_engine **out);
int ttx_mode_apply_dev(ttx_engine *h, const int32_t *m, const double *A_dev, int32_t mode, ttx_engine **out);
int ttx_mode_apply_last(const ttx_engine *h, double *ms, double *bytes_read, double *bytes_written, double *flops, int32_t *mode_ran);

/* The resident train in a function basis at a batch of REAL points, on the device (ttcross_amd/csrc/ttx_basis.h):
 *   f(x_p) = sum_i T(i_1 .. i_d) prod_m phi_(m, i_m)(x_(p, m)),
 * e.g. the density behind a train of COS-method coefficients (test_crs_coscoeff) or the piecewise-linear interpolant of a train of
 * grid values, at scattered points.  The train is not modified; no core crosses the host link.
 * Definition (numpy restates it: tests/basis_ref.py).  phi_m(p, :) is the table row of mode m and point p, n_m numbers.  The chain
 * runs from the last mode to the first, as dtt_ijk does:
 *   x = (1);  for mode i = d .. 1:  t_j(a) = sum_k U_i(a, j, k) x(k), summed from 0.0 over ascending k;
 *                                   z(a) = sum_j phi_j t_j(a),        summed from 0.0 over ascending j;   x = z;
 *   the value is z(1) after mode 1.  Multiply and add are always separate (the library is built with -ffp-contract=off).
 * With unit vectors for phi this is the chain of ttx_ijk_batch(.., TTX_EVAL_EXACT): 0.0 + 1.0 * t adds nothing to it.
 *   mode : TTX_EVAL_EXACT  the definition's operation order, one wave per point: bit-identical to the numpy restatement
 *          TTX_EVAL_MFMA   one chain step is the GEMM of the unfolded core r0 x (n r1) with the row-wise Kronecker product
 *                          phi_j(p) x_k(p), on the fp64 matrix cores: equal to EXACT to rounding.  A point's value depends on its
 *                          own table rows only, never on its neighbours, the chunk or npts; a call repeats bit for bit
 *          TTX_EVAL_AUTO   the engine chooses by the flops of the call (ttx_basis_last tells what ran)
 * Tables.  ttx_basis_batch forms them on the device from a ttx_basis per mode:
 *   TTX_BASIS_COS     y = (x - a) * w with w = pi / (b - a) (pi = 3.14159265358979323846); arg_j = (double)j * y;
 *                     phi_j = the project's own cosine (ttx_cos of ttcross_amd/csrc/ttx_coscoeff.h) of arg_j; phi_0 is multiplied by 0.5
 *                     with TTX_BASIS_HALVE_FIRST.  A non-finite coordinate or |arg_j| > 2^19 (TTX_TRIG_MAX) makes that phi_j NaN: the
 *                     point's value is NaN, the other points are untouched.
 *   TTX_BASIS_LINEAR  hat functions on n strictly ascending nodes t: n = 1: phi_0 = 1; x <= t_0: phi_0 = 1; x >= t_(n-1):
 *                     phi_(n-1) = 1; otherwise with i the last node with t_i <= x: lambda = (x - t_i) / (t_(i+1) - t_i),
 *                     phi_(i+1) = lambda, phi_i = 1.0 - lambda; every other entry 0.  A NaN coordinate gives a NaN row.  The table
 *                     is summed densely like any other (a two-term path is open).
 * ttx_basis_host writes the same tables on the host (no engine, no GPU): phi[j + n p] = phi_j(x[ldx p]); the device tables equal it
 * bit for bit.  ttx_basis_tab takes the caller's own tables, npts rows of sum n(k) numbers, mode 1 first.
 * The _dev entries take pointers on the engine's device, enqueue on the engine's stream and synchronise before they return;
 * ttx_basis_tab_dev reads the caller's table in place.  The basis descriptors (and their nodes) are always host memory.
 * Batches run in chunks of TTX_BASIS_CHUNK points (environment; default 2^18, 2^17 above maxrank 64); ttx_basis_tab stages at most
 * 2^25 table entries of host rows at a time.  The work space is the engine's own.
 * npts = 0 succeeds and launches nothing.  TTX_EINVAL: a null pointer with npts > 0, npts < 0, an unknown mode, an unknown kind,
 * b <= a or a non-finite a or b, nodes that are missing, not finite or not strictly ascending, ranks above 128.  TTX_ESTATE: no
 * train.  The engines are those ttx_ijk_batch takes: a multi-process engine is refused.
 * ttx_basis_last: of the last call on this engine, the milliseconds (HIP events) of the table launches and of the chain launches,
 * flops = 2 npts sum r(k-1) n(k) r(k), and the mode that ran (-1: none yet).  Any pointer may be NULL.
 * Open: the two-term LINEAR path, complex tables, ranks above 128.  The gradient is ttx_basis_grad_batch, below.
 * Added without a new ttx_version: look the symbols up. */
#define TTX_BASIS_COS    1   /* phi_j(x) = c_j cos(j pi (x - a)/(b - a)), j = 0..n-1; c_0 = 0.5 with TTX_BASIS_HALVE_FIRST, else 1 */
#define TTX_BASIS_LINEAR 2   /* hat functions on n strictly ascending nodes */
#define TTX_BASIS_HALVE_FIRST 1
typedef struct { int32_t kind, flags; double a, b; const double *nodes /* host, [n(k)], LINEAR only */; } ttx_basis;

int ttx_basis_batch    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const ttx_basis *basis /* [d] */, double *out, int32_t mode);
int ttx_basis_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, double *out_dev, int32_t mode);
int ttx_basis_tab      (ttx_engine *h, int64_t npts, const double *phi /* [npts][sum n(k)], mode 1 first */, double *out, int32_t mode);
int ttx_basis_tab_dev  (ttx_engine *h, int64_t npts, const double *phi_dev, double *out_dev, int32_t mode);
int ttx_basis_host     (const ttx_basis *b, int32_t n, int64_t npts, const double *x, int64_t ldx, double *phi /* [npts][n] */);   /* no engine, no GPU */
int ttx_basis_last     (const ttx_engine *h, double *ms_table, double *ms_chain, double *flops, int32_t *mode_ran);

/* Value and gradient of the same f at a batch of real points, on the device (ttcross_amd/csrc/ttx_basis_grad.h).  f is linear in every
 * table, so df/dx_m is the chain with mode m's table phi replaced by its derivative table dphi; with the states of one backward and
 * one forward pass all d partial derivatives cost about three value chains.  E.g. the score of the ttx_sample_sq_real proposal,
 * grad log q = 2 g grad g / (g^2 + gamma), from val = g and grad.
 * Definition (numpy restates it: tests/basis_grad_ref.py).  phi_i(p, :) and dphi_i(p, :) are the table rows of mode i, U_i(a, j, k) is
 * core i, r(i-1) x n(i) x r(i).  Multiply and add are always separate.
 *   Backward, i = d .. 1, from x = (1):  t_j(a) = sum_k U_i(a, j, k) x(k),                    summed from 0.0 over ascending k;
 *                                        z(a) = sum_j phi_j t_j(a), e(a) = sum_j dphi_j t_j(a), summed from 0.0 over ascending j;
 *                                        D_i = e;  x = z;   val = z(1) after mode 1: the operation sequence of ttx_basis_batch.
 *   Forward, i = 1 .. d, from l = (1):   grad_i = sum_a l(a) D_i(a),        summed from 0.0 over ascending a;
 *                                        s_j(k) = sum_a l(a) U_i(a, j, k),  summed from 0.0 over ascending a;
 *                                        l(k) <- sum_j phi_j s_j(k),        summed from 0.0 over ascending j (not formed after mode d).
 * val[npts] (may be NULL) is bit-identical to ttx_basis_batch / ttx_basis_tab on the same tables in the same effective mode, in
 * both modes.  grad[npts][d], mode 1 first (may not be NULL).
 *   mode : TTX_EVAL_EXACT  the order above, one wave per point: bit-identical to the numpy restatement
 *          TTX_EVAL_MFMA   both passes on the fp64 matrix cores: equal to EXACT to rounding.  A point's results depend on its own table
 *                          rows and on a fixed order only, never on its neighbours, the chunk, the store budget or npts; a call
 *                          repeats bit for bit
 *          TTX_EVAL_AUTO   by the flops of the call, 6 npts sum r(k-1) n(k) r(k) (ttx_basis_grad_last tells what ran)
 * Derivative tables.  ttx_basis_grad_batch forms phi as ttx_basis_batch does and dphi beside it:
 *   TTX_BASIS_COS     y, arg_j and the NaN rule of phi_j (a non-finite coordinate or |arg_j| > 2^19 makes dphi_j NaN); dphi_0 = 0.0;
 *                     otherwise dphi_j = -(((double)j * w) * sin(arg_j)) with the project's own sine (ttx_sin).  TTX_BASIS_HALVE_FIRST
 *                     touches j = 0 only, which is 0.0 anyway.
 *   TTX_BASIS_LINEAR  the derivative of the branch phi takes: a NaN coordinate gives a NaN row; n = 1, x <= t_0 or x >= t_(n-1): all
 *                     0.0; otherwise with i the last node with t_i <= x and s = 1.0 / (t_(i+1) - t_i): dphi_(i+1) = s, dphi_i = -s,
 *                     every other entry 0.0.  At an interior node this is the RIGHT-HAND derivative; on and outside the end nodes
 *                     the interpolant is constant and the derivative 0.
 * ttx_basis_host_d writes the same derivative tables on the host (no engine, no GPU), dphi[j + n p] = dphi_j(x[ldx p]); the device
 * tables equal it bit for bit.  ttx_basis_grad_tab takes the caller's own tables, two arrays in ttx_basis_tab's layout: any
 * differentiable basis works.  The _dev entries are as for ttx_basis_batch_dev.
 * The backward pass keeps D_i of every mode of a chunk, S = sum_k r(k-1) doubles per point.  A chunk is the smaller of
 * TTX_BASIS_CHUNK (or its default) and the largest multiple of 256 points with 8 S chunk <= TTX_BASIS_GRAD_STORE bytes (environment;
 * default 2^32), at least 256.  Argument checks and refusals are those of ttx_basis_batch.
 * ttx_basis_grad_last: of the last call on this engine, the milliseconds (HIP events) of the table, backward and forward launches,
 * flops = 6 npts sum r(k-1) n(k) r(k), the mode that ran (-1: none yet) and the points per chunk.  Any pointer may be NULL.
 * Open: second derivatives, a fused score entry for the samplers, ranks above 128.  The gradient with respect to the cores is
 * ttx_basis_core_grad_batch, below.
 * Added without a new ttx_version: look the symbols up. */
int ttx_basis_grad_batch    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const ttx_basis *basis /* [d] */, double *val, double *grad /* [npts][d] */, int32_t mode);
int ttx_basis_grad_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, double *val_dev, double *grad_dev, int32_t mode);
int ttx_basis_grad_tab      (ttx_engine *h, int64_t npts, const double *phi, const double *dphi /* [npts][sum n(k)] each */, double *val, double *grad, int32_t mode);
int ttx_basis_grad_tab_dev  (ttx_engine *h, int64_t npts, const double *phi_dev, const double *dphi_dev, double *val_dev, double *grad_dev, int32_t mode);
int ttx_basis_host_d        (const ttx_basis *b, int32_t n, int64_t npts, const double *x, int64_t ldx, double *dphi /* [npts][n] */);   /* no engine, no GPU */
int ttx_basis_grad_last     (const ttx_engine *h, double *ms_table, double *ms_back, double *ms_fwd, double *flops, int32_t *mode_ran, int64_t *chunk_ran);

/* Gradient of the same f with respect to the CORES at a batch of real points, on the device (ttcross_amd/csrc/ttx_basis_core_grad.h):
 * what fitting or correcting the resident train from scattered data (x_p, y_p) needs, without a core leaving the device.  f is linear in
 * every core; c[p] is the caller's weight, the derivative of their loss with respect to f(x_p) (e.g. f(x_p) - y_p for least squares).
 * Definition (numpy restates it: tests/basis_core_grad_ref.py).  phi_i(p, :) is the table row of mode i and point p, U_i(a, j, k) is core
 * i, r(i-1) x n(i) x r(i).  Multiply and add are always separate.
 *   Backward, i = d .. 1, from X_d = (1):  t_j(a) = sum_k U_i(a, j, k) X_i(k),   summed from 0.0 over ascending k;
 *                                          X_(i-1)(a) = sum_j phi_j t_j(a),     summed from 0.0 over ascending j;
 *                                          val = X_0(1): the operation sequence of ttx_basis_batch, every X_i kept.
 *   Forward, i = 1 .. d, from L_1 = (1):   s_j(k) = sum_a L_i(a) U_i(a, j, k),   summed from 0.0 over ascending a;
 *                                          L_(i+1)(k) = sum_j phi_j s_j(k),     summed from 0.0 over ascending j: the forward step of
 *                                          ttx_basis_grad_batch; L_(d+1) is not formed.
 *   Gradient:  G_i(a, j, k) = G0_i(a, j, k) + sum_p ((c[p] * L_i(p, a)) * (phi_(i, j)(p) * X_i(p, k))),  the terms added one by one over
 *              ascending p onto G0, the three multiplies bracketed as written.  G0 is 0.0 (accumulate == 0) or the contents of g on
 *              entry (accumulate == 1).
 * For any block E of core i's shape, sum_p c[p] f_(U_i <- E)(x_p) = <G_i, E>: the gradient of sum_p c[p] f(x_p), free of differences.
 * g holds the blocks in the layout of ttx_from_tt's cores: compact column-major, (a, j, k) at a + r(i-1) (j + n(i) k), mode 1 first,
 * sum_i ttx_core_size(h, i) doubles, all offsets 64-bit.  val[npts] may be NULL.
 *   mode : TTX_EVAL_EXACT  val and every G_i bit-identical to the numpy restatement: independent of the chunk, of the grid and of
 *                          repetition (each chunk continues from the buffer)
 *          TTX_EVAL_MFMA   both chains and the accumulation on the fp64 matrix cores.  val is bit-identical to ttx_basis_batch in MFMA
 *                          mode; G equals EXACT to rounding (tests/basis_core_grad_ref.py derives the allowance), in a fixed summation
 *                          order: no floating-point atomics, a call repeats bit for bit.  The order -- the chunks, and inside a chunk
 *                          segments of points whose partial blocks are added in ascending order -- depends on the train's shape and on
 *                          the points per chunk (TTX_BASIS_CHUNK, TTX_BASIS_GRAD_STORE), so G MAY DEPEND ON THE POINTS PER CHUNK, and on
 *                          nothing else the caller does not control: not on the device, and on npts only where npts is the points per chunk
 *          TTX_EVAL_AUTO   by the flops of the call, 6 npts sum r(k-1) n(k) r(k) (ttx_basis_core_grad_last tells what ran); the
 *                          break-even is provisional, not measured
 * Arguments, refusals and engine kinds are those of ttx_basis_batch (ranks up to 128, boundary ranks 1, no multi-process engine,
 * TTX_ESTATE without a train); in addition a NULL c or g with npts > 0 and an accumulate other than 0 or 1 are refused.  A refused call
 * leaves g untouched.  npts == 0 with accumulate == 0 writes 0.0 to all of g, with accumulate == 1 it touches nothing; neither launches
 * a chain.  A point with a NaN table entry or a NaN c[p] makes every entry of G it reaches NaN; 0 * NaN is NaN, so a point masked
 * with c[p] = 0 still needs finite coordinates (finite tables).
 * The backward chain keeps X_1 .. X_(d-1) of a chunk at the row stride of the value chain's kernels, S = (d - 1) ldx doubles per point
 * (ldx: the largest rank rounded up to four); the chunk rule is ttx_basis_grad_batch's with this S.
 * ttx_basis_core_grad_last: of the last call on this engine, the milliseconds (HIP events) of the table, backward, forward and
 * accumulation launches, the flops, the mode that ran (-1: none yet) and the points per chunk.  Any pointer may be NULL.
 * ttx_cores_axpy: U_i <- U_i + alpha[i-1] * G_i for all cores in one launch, multiply and add separate, g in the layout above.
 * alpha[i-1] == 0.0 skips core i without reading G_i: its bits stay even where G_i holds NaN.  The engine keeps nothing between calls
 * that is derived from the cores -- every operation (evaluation, norm, quadrature, sampling tables, Gram matrices) rebuilds what it
 * needs from the cores it finds, which is why ttx_ort and ttx_svd drop nothing either -- so nothing stale survives an update.  Refusals
 * as above, and a NULL alpha or g.
 * Open: second derivatives, ranks above 128, the Fortran layer.  The Gauss-Newton solver is ttx_basis_fit_batch, below; the gradient
 * of the normaliser Z of the squared density (maximum likelihood for ttx_sample_sq_real) is ttx_sq_lognorm_grad, further below.
 * Added without a new ttx_version: look the symbols up. */
int ttx_basis_core_grad_batch    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const ttx_basis *basis /* [d] */, const double *c /* [npts] */, double *val, double *g, int32_t accumulate, int32_t mode);
int ttx_basis_core_grad_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *c_dev, double *val_dev, double *g_dev, int32_t accumulate, int32_t mode);
int ttx_basis_core_grad_tab      (ttx_engine *h, int64_t npts, const double *phi /* [npts][sum n(k)] */, const double *c, double *val, double *g, int32_t accumulate, int32_t mode);
int ttx_basis_core_grad_tab_dev  (ttx_engine *h, int64_t npts, const double *phi_dev, const double *c_dev, double *val_dev, double *g_dev, int32_t accumulate, int32_t mode);
int ttx_basis_core_grad_last     (const ttx_engine *h, double *ms_table, double *ms_back, double *ms_fwd, double *ms_acc, double *flops, int32_t *mode_ran, int64_t *chunk_ran);
int ttx_cores_axpy    (ttx_engine *h, const double *alpha /* [d], host */, const double *g);
int ttx_cores_axpy_dev(ttx_engine *h, const double *alpha /* [d], host */, const double *g_dev);

/* Ranks grown from data: gradient enrichment (ttcross_amd/csrc/ttx_basis_enrich.h).  Everything above works at the ranks the train has;
 * this call appends to every bond the dominant directions of the TWO-SITE gradient that lie outside the range of the bond's left core,
 * and pads the right neighbour with zeros: the function does not change, and the next fit step can move into the new directions (the
 * enrichment of AMEn-style solvers and of rank-adaptive Riemannian completion).  The result is a NEW single-process engine without
 * integrand, as ttx_lincomb's; the source is untouched.  d >= 2.  phi, X_i, L_i and their operation orders are those of
 * ttx_basis_core_grad_batch; c[p] is the derivative of the caller's loss with respect to f(x_p); numpy restates all of it
 * (tests/enrich_ref.py).
 *  1. Directions per bond i = 1 .. d-1, on the host before any launch:
 *       k_i = max(0, min(add[i-1], r(i-1) n(i) - r(i), n(i+1) r(i+1), 128 - r(i))).
 *     (r(i) + k_i) times the largest mode must not exceed what a new engine stores (maxrank*n); a violation refuses the call.
 *  2. Sketch matrix Omega_i (k_i, n(i+1), r(i+1)), uniform on (-1, 1): entry (q, j, b) is ttx_lincomb_round's step-2 formula at
 *     (seed, k = i, x = q + k_i (j + n(i+1) b)).  It is generated where it is used and never stored.
 *  3. Sketch state z_q(p) = sum_j phi_(i+1, j)(p) t_j(q), t_j(q) = sum_b Omega_i(q, j, b) X_(i+1)(p, b): both sums from 0.0, over
 *     ascending b and ascending j -- the backward step of the value chain with Omega_i in place of a core.  X_d = (1).
 *  4. Sketch of the two-site gradient: Y_i(a, j, q) = sum_p ((c[p] * L_i(p, a)) * (phi_(i, j)(p) * z_q(p))), the terms added over ascending
 *     p from 0.0, brackets as written: G_i's formula with z for X_i.  Y_i = G2_i Omega_i^T for the two-site gradient
 *     G2_i = sum_p c_p (L_i (x) phi_i)(phi_(i+1) (x) X_(i+1))^T, which is never formed.
 *  5. Per bond, on the device: max |Y_i|, whether every entry is finite, ynorm2_i = sum Y^2 by ttx_cores_dot's rule with
 *     tot = r(i-1) n(i) k_i.  A bond whose sketch is all zero or not finite takes no direction: added = 0, its gain row 0.0 for a zero
 *     sketch and NaN for one that is not finite.  Otherwise added = k_i.
 *  6. New directions: Q_i = the columns r(i) + 1 .. r(i) + k_i of the explicit Householder Q of the tall matrix [U_i^L | 2^-e Y_i]
 *     (U_i^L the r(i-1) n(i) x r(i) unfolding, (f, e) = frexp(max |Y_i|)), by the engine's own QR, the one of ttx_lincomb_round's step 4.
 *     gain_i[q] = ldexp(|R(r(i) + q, r(i) + q)|, e).  The first r(i) columns of Q span a space that contains range(U_i^L), so Q_i is
 *     orthonormal and orthogonal to it, also when U_i^L is rank-deficient.
 *  7. New core i, shape (r(i-1) + added(i-1), n(i), r(i) + added(i)): block [:r(i-1), :, :r(i)] is U_i bit for bit, block
 *     [:r(i-1), :, r(i):] is Q_i, all rows from r(i-1) on are 0.0.
 * The new train is the same function: in exact mode its value chain equals the source's at any point with a finite chain, the
 * enlargement adds only x + 0.0 and 0.0 * y terms.  At a stationary point of a fixed-rank fit Y_i is already orthogonal to
 * range(U_i^L), so sum_q gain_i[q]^2 is about ynorm2_i; away from one, step 6 removes the part the one-site gradient already reaches.
 * Q_i is defined up to what a Householder QR leaves open (signs, and the basis inside the span when k_i > 1 matters only through R).
 *   mode : TTX_EVAL_EXACT  Y, ynorm2 and the copied blocks bit for bit the numpy restatement; independent of TTX_BASIS_CHUNK /
 *                          TTX_BASIS_GRAD_STORE, of the grid and of repetition
 *          TTX_EVAL_MFMA   steps 3 and 4 on v_mfma_f64_16x16x4_f64; segment sums in a fixed order, no atomics, a call repeats bit for
 *                          bit; Y within the allowance of tests/enrich_ref.py (ttx_basis_core_grad's count with the Omega step)
 *          TTX_EVAL_AUTO   by the flops of the call, npts (4 sum r n r + 2 sum_i k_i (n(i+1) r(i+1) + r(i-1) n(i))), against a
 *                          PROVISIONAL break-even (TTX_EN_AUTO_FLOPS; TTX_ENRICH_AUTO_FLOPS in the environment replaces it)
 * Steps 5 - 7 are the same in both modes.  Every state row of the call (X, L, z) has the stride ldx = max(r, k) rounded up to four; the
 * chunk rule is ttx_basis_core_grad_batch's with S = d ldx doubles per point (the states and the chunk's z block).
 * added[d-1], gain[d-1][128] (unused entries 0), ynorm2[d-1] and y (the packed Y_i in bond order, (a, j, q) at a + r(i-1) (j + n(i) q),
 * with the k_i of step 1 also where added is 0; on the device for the _dev entries) may each be NULL.
 * Refusals: those of ttx_basis_core_grad_batch; a NULL add or out; a NULL c with npts > 0; a negative add; the storage check of step 1.
 * After a refusal *out is NULL.  npts == 0 gives a zero sketch on every bond: out is a plain copy.
 * ttx_basis_enrich_last: of the last call on this engine, the milliseconds (HIP events) of the table, backward, sketch (forward
 * advance, z, Y and statistics), QR and assembly launches, the flops, the mode that ran (-1: none yet), the points per chunk.
 * Open: growth of the source engine in place, the normaliser's two-site term for the squared density, power iterations on the sketch,
 * ranks above 128.  Added without a new ttx_version: look the symbols up. */
int ttx_basis_enrich_batch    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const ttx_basis *basis /* [d] */, const double *c /* [npts] */, const int32_t *add /* [d-1] */,
                               uint64_t seed, int32_t mode, ttx_engine **out, int32_t *added /* [d-1] */, double *gain /* [d-1][128] */, double *ynorm2 /* [d-1] */, double *y);
int ttx_basis_enrich_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *c_dev, const int32_t *add,
                               uint64_t seed, int32_t mode, ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y_dev);
int ttx_basis_enrich_tab      (ttx_engine *h, int64_t npts, const double *phi /* [npts][sum n(k)] */, const double *c, const int32_t *add,
                               uint64_t seed, int32_t mode, ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y);
int ttx_basis_enrich_tab_dev  (ttx_engine *h, int64_t npts, const double *phi_dev, const double *c_dev, const int32_t *add,
                               uint64_t seed, int32_t mode, ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y_dev);
int ttx_basis_enrich_last     (const ttx_engine *h, double *ms_table, double *ms_back, double *ms_sketch, double *ms_qr, double *ms_asm, double *flops, int32_t *mode_ran, int64_t *chunk_ran);

/* Derivative of the same f along a direction V in core space, at a batch of real points (ttcross_amd/csrc/ttx_basis_jvp.h): J V, cores
 * to points, the other half of ttx_basis_core_grad_batch (J^T c, points to cores).  With both, a Gauss-Newton or Levenberg-Marquardt
 * step is solved matrix-free; a JVP keeps no states, so its point count is not limited by a state store.
 *     dval_p = sum_i f_(U_i <- V_i)(x_p)
 * v has the packed layout of g in ttx_basis_core_grad_batch (mode 1 first, (a, j, k) at a + r(i-1) (j + n(i) k)); it is read in place.
 * Definition (numpy restates it: tests/basis_jvp_ref.py).  Multiply and add are always separate.  Backward, i = d .. 1, from X = (1),
 * Y = (0.0):
 *     t_j(a) = sum_k U_i(a,j,k) X(k),  s_j(a) = sum_k U_i(a,j,k) Y(k),  v_j(a) = sum_k V_i(a,j,k) X(k)   each from 0.0 over ascending k
 *     z(a)   = sum_j phi_j t_j(a),     y(a)   = sum_j phi_j (s_j(a) + v_j(a))                            each from 0.0 over ascending j
 *     X <- z,  Y <- y;   val = z(1) and dval = y(1) after mode 1.  The Y term of mode d is formed like any other.
 * val[npts] may be NULL; it is the operation sequence of ttx_basis_batch and bit-identical to it in the same effective mode.
 *   mode : TTX_EVAL_EXACT  the order above, one wave per point: bit-identical to the restatement
 *          TTX_EVAL_MFMA   equal to EXACT to rounding (tests/basis_jvp_ref.py derives the bound).  A point's results depend on its own
 *                          table rows only: never on its neighbours, the chunk (TTX_BASIS_CHUNK) or npts.  A call repeats bit for bit.
 *          TTX_EVAL_AUTO   by 6 npts sum r(k-1) n(k) r(k) against a PROVISIONAL break-even (that of ttx_basis_batch; not measured)
 * Arguments, refusals and engine kinds are those of ttx_basis_batch; in addition a NULL v or dval with npts > 0 is refused.  npts == 0
 * launches nothing.  A point with a NaN table entry has val = dval = NaN, and no other point has.
 * ttx_basis_jvp_last: of the last call on this engine, the milliseconds of the table and chain launches, the flops, the mode that ran.
 *
 * Vector operations on packed core-space buffers, for a caller's own optimiser (momentum, Adam, a line search) and the solver below.
 * ttx_cores_dot: sum_e a_e * b_e in a fixed order that does not depend on the device and repeats bit for bit (numpy restates it).
 *   With tot = sum_i ttx_core_size(h, i) the buffer is cut into 256 segments of L = 256 * ceil(tot / 65536) elements (the last ones may
 *   be short or empty); inside a segment lane t sums the products of its elements e = t (mod 256) in ascending order from 0.0; the 256
 *   lane sums are halved (t, t + 128), (t, t + 64), .. (0, 1); the 256 segment sums are added in ascending order from 0.0.
 * ttx_cores_axpby_dev: y_e <- (alpha * x_e) + (beta * y_e), two multiplies and one add, no special cases; x and y on the engine's device.
 * ttx_cores_get_dev / ttx_cores_set_dev (ttx_cores_get / ttx_cores_set: a host buffer): the engine's cores to and from a packed
 *   buffer of the present ranks, bit for bit.  After a set
 *   nothing stale survives, as after ttx_cores_axpy: the engine keeps nothing between calls that is derived from the cores.
 * Refusals: those of ttx_cores_axpy, and a NULL buffer or out.
 *
 * ttx_basis_fit_batch / _tab: minimise loss = 1/2 sum_p w_p (f(x_p) - y_p)^2 over all cores of the resident train, in place, by a
 * matrix-free Levenberg-Marquardt iteration (the controller is ttcross_amd/csrc/ttx_fit_plan.h; tests/basis_jvp_ref.py: fit_numpy
 * restates the whole solver).  Every scalar operation is one host double operation in the order written; sums over core space are
 * ttx_cores_dot's, sums over the points the same rule with tot = npts.
 *   1. val = f(x_p), res = val - y, c = w * res, loss = 0.5 * dot_n(c, res); g = J^T c; rho0 = dot(g, g); rho0 == 0 stops (reason 3).
 *      A rejected step leaves the cores, and so g and loss, as they were: they are kept, not formed again.
 *   2. CG on (J^T W J + lambda I) s = -g:  s = 0, r = (-1 * g) + (1 * 0), p = r, rho = rho0.
 *   3. For k < cg_max:  q = J p;  Ap = J^T (w * q);  Ap <- (lambda * p) + (1 * Ap);  pAp = dot(p, Ap);  leave the loop unless pAp is a
 *      positive finite number;  alpha = rho / pAp;  s <- (alpha * p) + (1 * s);  r <- (-alpha * Ap) + (1 * r);  rho_new = dot(r, r);
 *      stop the loop where rho_new <= (cg_tol * cg_tol) * rho0;  p <- (1 * r) + ((rho_new / rho) * p);  rho = rho_new.
 *   4. Snapshot the cores (ttx_cores_get_dev), ttx_cores_axpy(1.0, s), the trial loss by the value chain.
 *   5. Accepted where the trial loss is finite and strictly smaller: lambda *= lambda_down.  Otherwise the snapshot is copied back
 *      (not subtracted: that would not give the bits back) and lambda *= lambda_up.  A loop that ended with s = 0 is a rejection.
 * w NULL means all ones (c = res, Ap = J^T q); a negative or non-finite w (host forms) is refused.  The host forms upload x (or the
 * table), y and w once; every pass then runs the _dev paths.  History, each array may be NULL: loss[max_iter + 1] (loss[0] at entry,
 * loss[i + 1] after iteration i), lambda[max_iter] (what iteration i solved with), cg_iters[max_iter] (its J V products),
 * accepted[max_iter]; entries past result->iters repeat the last loss and lambda with cg_iters = accepted = 0.
 * TTX_EVAL_EXACT follows fit_numpy bit for bit; TTX_EVAL_MFMA runs every chain on the matrix cores; TTX_EVAL_AUTO decides per call.
 * Refusals: those of ttx_basis_core_grad_batch (multi-process engines, ranks, TTX_ESTATE), a NULL opts, y or input with npts > 0,
 * npts < 1, options out of range (max_iter < 0, cg_max < 1, max_reject < 1, lambda0 <= 0, lambda_down outside (0, 1], lambda_up < 1,
 * negative tolerances); work space that cannot be allocated is TTX_EHIP, nothing faults.  A refused call leaves the cores untouched.
 * ttx_basis_fit_last: of the last fit on this engine, the milliseconds in JVP, core-gradient, value and vector launches, the counts of
 * JVP and core-gradient calls, the mode the last JVP ran in (-1: none).
 * Open: an ALS sweep, rank adaptation during the fit, a preconditioner for CG, ranks above 128.  (Maximum likelihood for the squared
 * density: ttx_sq_nll_batch, below.)
 * Added without a new ttx_version: look the symbols up. */
typedef struct { int32_t max_iter, cg_max, max_reject, mode; double lambda0, lambda_down, lambda_up, cg_tol, loss_tol; } ttx_fit_opts;
typedef struct { int32_t iters, stop; /* 1 max_iter, 2 loss_tol, 3 zero gradient, 4 max_reject consecutive rejections, 5 non-finite loss at entry */ } ttx_fit_result;
int ttx_basis_jvp_batch    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const ttx_basis *basis /* [d] */, const double *v, double *val, double *dval, int32_t mode);
int ttx_basis_jvp_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *v_dev, double *val_dev, double *dval_dev, int32_t mode);
int ttx_basis_jvp_tab      (ttx_engine *h, int64_t npts, const double *phi /* [npts][sum n(k)] */, const double *v, double *val, double *dval, int32_t mode);
int ttx_basis_jvp_tab_dev  (ttx_engine *h, int64_t npts, const double *phi_dev, const double *v_dev, double *val_dev, double *dval_dev, int32_t mode);
int ttx_basis_jvp_last     (const ttx_engine *h, double *ms_table, double *ms_chain, double *flops, int32_t *mode_ran);
int ttx_cores_dot      (ttx_engine *h, const double *a, const double *b, double *out);
int ttx_cores_dot_dev  (ttx_engine *h, const double *a_dev, const double *b_dev, double *out /* host */);
int ttx_cores_axpby_dev(ttx_engine *h, double alpha, const double *x_dev, double beta, double *y_dev);
int ttx_cores_get      (ttx_engine *h, double *g);
int ttx_cores_set      (ttx_engine *h, const double *g);
int ttx_cores_get_dev  (ttx_engine *h, double *g_dev);
int ttx_cores_set_dev  (ttx_engine *h, const double *g_dev);
int ttx_basis_fit_batch    (ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, const double *y, const double *w, const ttx_fit_opts *opts,
                            double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result);
int ttx_basis_fit_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *y_dev, const double *w_dev, const ttx_fit_opts *opts,
                            double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result);
int ttx_basis_fit_tab      (ttx_engine *h, int64_t npts, const double *phi, const double *y, const double *w, const ttx_fit_opts *opts,
                            double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result);
int ttx_basis_fit_tab_dev  (ttx_engine *h, int64_t npts, const double *phi_dev, const double *y_dev, const double *w_dev, const ttx_fit_opts *opts,
                            double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result);
int ttx_basis_fit_last     (const ttx_engine *h, double *ms_jvp, double *ms_core_grad, double *ms_value, double *ms_vector, int64_t *n_jvp, int64_t *n_core_grad, int32_t *mode_ran);

/* The normaliser of the squared density q(x) = (f(x)^2 + gamma) / (Z + gamma V), its logarithm and its gradient with respect to the
 * cores, on the device (ttcross_amd/csrc/ttx_sq_norm.h): the half of a maximum-likelihood step that ttx_basis_core_grad_batch does not
 * give.  Z = <f, f>_M = sum T(i_1 .. i_d) M_1(i_1, i'_1) .. M_d(i_d, i'_d) T(i'_1 .. i'_d) with one symmetric tridiagonal matrix per mode:
 *   md[k][0 .. n_k-1] its diagonal, mo[k][i] = M_k(i, i+1), i = 0 .. n_k-2; a NULL mo or a NULL mo[k] means a diagonal matrix.  Host rows.
 * That covers the diagonal weights of ttx_sample_sq, the hat functions' mass matrix of ttx_sample_sq_real, a held mode (phi phi^T of its
 * two adjacent hat values) and the identity of an orthonormal basis.  gvol >= 0 is the caller's gamma * V.
 * Definition (numpy restates it: tests/sq_norm_ref.py).  U_k(a, i, b) is core k; multiply and add are always separate; every sum
 * starts from 0.0 and runs over ascending indices.
 *   V_k(a, i, b) = ((0.0 + mo(i-1) * U_k(a, i-1, b)) + md(i) * U_k(a, i, b)) + mo(i) * U_k(a, i+1, b): the terms i-1, i, i+1 in this order,
 *                  a term that does not exist (i = 0, i = n-1, a diagonal matrix) is left out
 *   Right chain, k = d .. 2, from PR_d = [1], eR(d) = 0:
 *       Y(a', i, b) = sum_b' PR_k(b, b') * V_k(a', i, b');   p_i(a, a') = sum_b U_k(a, i, b) * Y(a', i, b);   PR_(k-1) = sum_i p_i
 *   Left chain, k = 1 .. d, from PL_0 = [1], eL(0) = 0:
 *       W_k(a, i, b') = sum_a' PL_(k-1)(a, a') * V_k(a', i, b');   p_i(b, b') = sum_a U_k(a, i, b) * W_k(a, i, b');   PL_k = sum_i p_i
 *   (every p_i is summed on its own from 0.0, then the p_i are added over ascending i from 0.0: a step is as wide as the core is long)
 *   After every step the new matrix is multiplied by 2^-ex, ex the exponent that takes its largest entry in magnitude into [0.5, 1)
 *   (frexp; ex = 0 where that entry is 0 or not finite: ttx_sample_sq's rule), and eR(k-1) = eR(k) + ex, eL(k) = eL(k-1) + ex.
 *   z_mant = PL_d, z_exp = eL(d):  Z = z_mant 2^z_exp.   den = z_mant + ldexp(gvol, -z_exp);   logz = z_exp * ln 2 + log(den) = log(Z + gvol).
 *   D_k(a, i, b) = sum_b' W_k(a, i, b') * PR_k(b, b');   s_k = ldexp((2 * coef) / den, eL(k-1) + eR(k) - z_exp);
 *   G_k(a, i, b) = G0_k(a, i, b) + s_k * D_k(a, i, b)  =  G0_k + (coef / (Z + gvol)) dZ/dU_k,  formed from the scaled quantities: nothing
 *   overflows where Z does.  G0 is 0.0 (accumulate == 0) or the contents of g on entry (accumulate == 1); g in the packed layout of
 *   ttx_basis_core_grad_batch.  coef = 1 gives the gradient of log(Z + gvol).
 * Euler: <dZ/dU_k, U_k> = 2 Z for every k.  For a block E of core k's shape <dZ/dU_k, E> = 2 <T, T_(U_k <- E)>_M.
 *   mode : TTX_EVAL_EXACT  z_mant, z_exp and every G_k bit-identical to the restatement
 *          TTX_EVAL_MFMA   the assembly D_k = W_k PR_k^T of all cores on the fp64 matrix cores, one launch; the chains are EXACT's, so
 *                          z_mant, z_exp and logz are the same bits and G equals EXACT to rounding (sq_norm_ref.py derives the
 *                          allowance); no floating-point atomics, a call repeats bit for bit
 *          TTX_EVAL_AUTO   by the flops of the call, sum 4 r0^2 n r1 + 6 r0 n r1^2, against a PROVISIONAL break-even
 * No special cases: a Z + gvol that is zero, negative or not finite gives what the arithmetic gives; a NaN core gives NaN; nothing
 * faults.  Work space: one buffer of the size of g (every W_k), sum r_k^2 doubles (every PR_k), one core (Y), max n_k r^2 doubles (the p_i of a step).
 * Refusals: those of ttx_cores_axpy (no train: TTX_ESTATE; a multi-process engine; ranks above 128; boundary ranks; a NULL g), a NULL md
 * or md[k], a non-finite entry of md or mo, gvol negative or not finite, coef not finite, accumulate not 0 or 1, an unknown mode.  A
 * refused call leaves g untouched.  z_mant, z_exp and logz may be NULL.
 * ttx_sq_lognorm_grad_last: of the last call on this engine, the milliseconds of the right chain, the left chain and the assembly, the
 * flops and the mode that ran (-1: none yet).
 *
 * ttx_sq_nll_batch: the negative log-likelihood of weighted points under q and its gradient with respect to the cores, in one call.
 *   val_p = f(x_p): ttx_basis_batch's value chain, bit for bit (a value chain of its own: c depends on val, and the core gradient's
 *           backward pass forms val only together with the states its forward pass consumes, so the call costs one extra value chain);
 *   c_p = -((2 * w_p) * val_p) / (val_p * val_p + gamma);   l_p = log(val_p * val_p + gamma);   w NULL: all ones;
 *   S = sum_p w_p * l_p and Wsum = sum_p w_p * 1.0 by ttx_cores_dot's rule with tot = npts;
 *   G = J^T c (ttx_basis_core_grad_batch_dev, accumulate 0), then ttx_sq_lognorm_grad_dev with coef = Wsum and accumulate = 1;
 *   nll = -S + Wsum * logz.
 * val may be NULL.  A point with val^2 + gamma = 0 makes nll +inf and G NaN by the arithmetic: an optimiser rejects the step.
 * npts == 0 gives nll = 0 * logz and G = 0 * D.  Each of the three parts takes mode on its own (AUTO by its own flops).
 * Refusals: those of ttx_basis_core_grad_batch and of ttx_sq_lognorm_grad, a NULL nll, g or basis, a negative or non-finite gamma,
 * and in the host form a negative or non-finite w.  Open: a table form, per-call reuse of the chains in a line search, a Hessian of Z,
 * ranks above 128, the Fortran layer.  Added without a new ttx_version: look the symbols up. */
int ttx_sq_lognorm_grad     (ttx_engine *h, const double *const *md, const double *const *mo, double gvol, double coef, double *g, int32_t accumulate, int32_t mode, double *z_mant, int64_t *z_exp, double *logz);
int ttx_sq_lognorm_grad_dev (ttx_engine *h, const double *const *md, const double *const *mo, double gvol, double coef, double *g_dev, int32_t accumulate, int32_t mode, double *z_mant, int64_t *z_exp, double *logz);
int ttx_sq_lognorm_grad_last(const ttx_engine *h, double *ms_right, double *ms_left, double *ms_asm, double *flops, int32_t *mode_ran);
int ttx_sq_nll_batch    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const ttx_basis *basis /* [d] */, const double *w, double gamma, const double *const *md, const double *const *mo,
                         double gvol, int32_t mode, double *nll, double *logz, double *val, double *g);
int ttx_sq_nll_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *w_dev, double gamma, const double *const *md, const double *const *mo,
                         double gvol, int32_t mode, double *nll, double *logz, double *val_dev, double *g_dev);

/* Moments and one-mode reduced density matrices of the squared density, on the device (ttcross_amd/csrc/ttx_sq_moments.h): what reads a
 * fitted q = (f^2 + gamma) / (Z + gamma V).  With symmetric tridiagonal observables A_k (ad, ao) and A2_k (a2d, a2o), rows as md and mo:
 *   m1[l]    = <f, A_l f>_M / Z                 (A_l at mode l, M_j at every other mode)
 *   c2[k][l] = <f, (A_k x A_l) f>_M / Z, k != l;  c2[k][k] = <f, A2_k f>_M / Z (0.0 where A2_k is not given)
 *   bd, bo   = the band of B_k / Z, B_k(i, i') = sum PL_(k-1)(a, a') U_k(a', i, b') PR_k(b, b') U_k(a, i', b): sum_ii' B_k(i, i') X(i, i') / Z is
 *              the moment of any one-mode X, and phi(x)^T B_k phi(x) / Z the marginal density of f^2 / Z in mode k for hat functions phi
 * all ratios that stay O(1) where Z leaves the double range.  ad NULL: no moments asked (m1 and c2, where given, are filled with 0.0);
 * ad[k] NULL: mode k is not selected, its m1 and its rows and columns of c2 are 0.0; ao or ao[k] NULL: A_k is diagonal; the same for a2d, a2o.
 * bd and bo are [sum n_k] each, mode k's row at n_1 + .. + n_(k-1), bo[k][n_k - 1] = 0.0; the band is formed only where both are given.
 * m1 is [d], c2 [d][d]; each of z_mant, z_exp, bd / bo, m1, c2 may be NULL, not all of them.
 * Definition (numpy restates it: tests/sq_moments_ref.py), in the terms of ttx_sq_lognorm_grad above; "left step with X from P" is one step
 * of its left chain with X in place of M_k and P in place of PL_(k-1), "right step" the same for the right chain; every p_i on its own, the
 * p_i added over ascending i from 0.0.
 *   1. The chains of ttx_sq_lognorm_grad: PL_k, eL(k), PR_k, eR(k), z_mant, z_exp -- the same bits.
 *   2. RA_(l-1) for a selected l: the right step with A_l from PR_l, the sum of the p_i NOT rescaled; exponent eR(l).
 *   3. m1[l] = ldexp(dot(PL_(l-1), RA_(l-1)) / z_mant, eL(l-1) + eR(l) - z_exp), dot the sum of the entrywise products of the two column-major
 *      matrices by ttx_cores_dot's rule with tot = r_(l-1)^2; the exponent clamped to +-100000.  c2[l][l]: the same with A2_l.
 *   4. C^(k)_k for a selected k below the largest selected mode: the left step with A_k from PL_(k-1), then the power-of-two rule, exponent
 *      e^(k)_k = eL(k-1) + ex; C^(k)_j, j = k+1 .. l_max - 1 (l_max the largest selected mode): the left step with M_j from C^(k)_(j-1), the rule,
 *      e^(k)_j = e^(k)_(j-1) + ex.
 *   5. c2[k][l] = c2[l][k] = ldexp(dot(C^(k)_(l-1), RA_(l-1)) / z_mant, e^(k)_(l-1) + eR(l) - z_exp) for selected k < l.
 *   6. T(a, i, b') = sum_a' PL_(k-1)(a, a') * U_k(a', i, b');  D0(a, i, b) = sum_b' T(a, i, b') * PR_k(b, b');
 *      B_k(i, i') = sum_b [ sum_a U_k(a, i, b) * D0(a, i', b) ];  bd[k][i] = ldexp(B_k(i, i) / z_mant, eL(k-1) + eR(k) - z_exp), bo[k][i] of B_k(i, i+1).
 *   mode : TTX_EVAL_EXACT  every output bit-identical to the restatement
 *          TTX_EVAL_MFMA   the left steps of item 4 on the fp64 matrix cores: W = C V for all carried matrices of a mode in one launch,
 *                          P = U^T W summed over (a, i) in one accumulation; items 1, 2, 3, 6, the power-of-two rule and every dot are
 *                          EXACT's kernels, so z_mant, z_exp, m1, the diagonal of c2, bd and bo are the same bits and the off-diagonal of c2
 *                          agrees to rounding (sq_moments_ref.py derives the allowance); no floating-point atomics, a call repeats bit for bit
 *          TTX_EVAL_AUTO   by the flops of the call against a PROVISIONAL break-even (TTX_SQM_AUTO_FLOPS, also read from the environment)
 * The carried matrices of a mode go through one launch per kernel, cut into batches so that the work space of a launch stays under
 * TTX_SQM_CAP_BYTES (ttx_op_plan.h); TTX_SQM_BATCH in the environment lowers the batch.  A carried matrix does not depend on the cut.
 * A NaN core gives NaN; nothing faults; work space that cannot be allocated is TTX_EHIP.
 * Refusals: those of ttx_sq_lognorm_grad (no train: TTX_ESTATE; a multi-process engine; ranks above 128; boundary ranks; a NULL md or md[k];
 * a non-finite entry of md or mo), a non-finite entry of ad, ao, a2d or a2o, an unknown mode, every output NULL.  A refused call writes nothing.
 * ttx_sq_moments_last: of the last call on this engine, the milliseconds of the chains, the band, the carried steps and the closing
 * products (with the right matrices), the flops, the number of carried chain steps sum_k (l_max - k) and the mode that ran (-1: none yet).
 * Open: two-mode marginal densities, higher moments, ranks above 128.  Added without a new ttx_version: look the symbols up. */
int ttx_sq_moments(ttx_engine *h,
    const double *const *md, const double *const *mo,
    const double *const *ad, const double *const *ao,
    const double *const *a2d, const double *const *a2o,
    int32_t mode,
    double *z_mant, int64_t *z_exp,
    double *bd, double *bo,
    double *m1 /* [d] */, double *c2 /* [d][d] */);
int ttx_sq_moments_last(const ttx_engine *h, double *ms_chains, double *ms_band, double *ms_carry, double *ms_close, double *flops, int64_t *steps, int32_t *mode_ran);

/* Samples drawn from the resident train by sequential conditional sampling, on the device (ttcross_amd/csrc/ttx_sample.h).
 * Modes are 1-based, G_k is core k, r_0 = r_d = 1.
 *   u     : npts rows of d uniforms, row-major [npts][d]; u_k draws mode k
 *   w     : d blocks of n_k weights as for ttx_quad; NULL = all ones
 *   fixed : d entries, 0 = the mode is drawn, f in 1..n_k = the mode is held at index f (its u_k is not looked at); NULL = all drawn
 *   ind   : [npts][d], 1-based, the layout ttx_ijk_batch reads;  logq, val : [npts], each may be NULL
 * Definition.  Effective weight e_k(i): w_k(i) for a drawn mode; for a fixed mode 1 at i = f_k and 0 elsewhere (the quadrature
 * weight of a fixed mode does not enter).  Prefix vectors: l_0 = [1], l_k = l_(k-1) M_k with M_k = sum_i e_k(i) G_k(:, i, :), formed
 * by the kernels of ttx_marginals in their summation order.  Head table of a drawn mode: H_k(i, b) = w_k(i) * sum_a l_(k-1)(a) G_k(a, i, b),
 * the sum over ascending a from 0.0 with a separate multiply and add, the weight multiplied in last.
 * Modes are drawn from the LAST to the first, so the running state is dtt_ijk's own chain.  x_(d+1) = [1]; for k = d .. 1:
 *   m_k(i) = sum_b H_k(i, b) x_(k+1)(b)  (ascending b from 0.0, separate multiply and add);  p_k(i) = |m_k(i)|
 *   c_k(i) = the inclusive running sum of p_k.  Its association order depends on i alone: indices are taken in blocks of 64,
 *            i = 64 j + l; inside a block s(l) is formed in six doubling steps o = 1, 2, 4, .. 32, s(l) <- s(l - o) + s(l) for l >= o
 *            (all l at once, from s = p), and c(64 j + l) = c(64 j - 1) + s(l), c(-1) = 0.  Not the grid, the chunk or the other
 *            samples enter.  In floating point such a sum need not be monotone, hence the p > 0 in the next line.
 *   t = u_k c_k(n_k);  i_k = the smallest i with p_k(i) > 0 and t < c_k(i); if there is none, or u_k >= 1, the largest i with
 *   p_k(i) > 0.  An index with p_k(i) = 0 is never chosen.  A fixed mode takes i_k = f_k and computes no p.
 *   x_k = G_k(:, i_k, :) x_(k+1) in the operation sequence of ttx_ijk_batch's TTX_EVAL_EXACT (sums from 0.0 over ascending b,
 *   separate multiply and add, two rows per lane above rank 64; x_d is a copy of G_d(:, i_d, 1)).
 * Outputs: ind = (i_1 .. i_d); val = x_1(1), the train's element at ind, equal bit for bit to ttx_ijk_batch(ind, TTX_EVAL_EXACT);
 * logq = sum over the drawn modes, k = d .. 1, of log(p_k(i_k) / c_k(n_k)): the log of the probability with which ind was drawn.
 * Distribution: for a train and weights without sign changes the samples follow |T(i)| w(i) / Z exactly, up to rounding.  For a
 * signed train they follow the product of the ABSOLUTE conditional marginals, which is not |T| w / Z: exp(logq) is the proposal
 * density to reweight with, E_q[val w(ind) / exp(logq)] = sum_i T(i) w(i) over the drawn modes at the fixed indices.
 * Failed samples: c_k(n_k) is 0, NaN or Inf at some mode, or the u_k of a drawn mode is NaN or negative (-0.0 counts as 0).  A
 * failed sample gets an index row of zeros, logq = NaN and val = 0.0, and is counted (ttx_sample_last); the others are untouched.
 * Safety: an index is formed from lane numbers, never from a value, so whatever the cores, weights and u hold (NaN included)
 * every index written lies in 0..n_k and no read leaves its table.  Arithmetic is plain double without a running exponent.
 * A mode of up to 1024 indices keeps its row of p in LDS, a longer one in a per-wave row of the call's global work space.
 * Samples go in chunks of TTX_SAMPLE_CHUNK (environment, default 2^18); the tables are built once per call; no atomics; a
 * sample does not depend on its neighbours or on the chunk, and a call repeats bit for bit.  The train is not modified; the work
 * space is the engine's own (the vectors of ttx_marginals are shared), allocated on first use and freed by ttx_destroy.
 * ttx_sample_dev: u, ind, logq and val are pointers on the engine's device, w and fixed stay host pointers; it enqueues on the
 * engine's stream and synchronises before it returns.  No sample crosses the host link: ind can go into ttx_ijk_batch_dev.
 * npts = 0 succeeds and launches nothing.  TTX_EINVAL: npts < 0, null u / ind with npts > 0 (both before the engine is looked
 * at), a fixed entry outside 0..n_k (before any device call), ranks above 128; TTX_ESTATE: an engine without a train; a
 * multi-process engine is refused as by ttx_ijk (a replica, ttx_replicate, is accepted).
 * ttx_sample_last: of the last call on this engine, the milliseconds (HIP events) of k_sm_head and of k_sm_draw (summed over the
 * chunks), the bytes of the cores k_sm_head read (8 sum r(k-1) n(k) r(k) over the drawn modes) and the failed samples; any
 * pointer may be NULL.  Added without a new ttx_version: look the symbols up. */
int ttx_sample(ttx_engine *h, int64_t npts, const double *u /* [npts][d] */, const double *w, const int32_t *fixed, int32_t *ind, double *logq, double *val);
int ttx_sample_dev(ttx_engine *h, int64_t npts, const double *u, const double *w, const int32_t *fixed, int32_t *ind, double *logq, double *val);
int ttx_sample_last(const ttx_engine *h, double *ms_head, double *bytes_head, double *ms_draw, int64_t *nfailed);

/* Samples drawn from the SQUARE of the resident train on the device (ttcross_amd/csrc/ttx_sample_sq.h): the squared-density sampler
 * (SIRT: Cui and Dolgov, 2022) on grid indices.  ttx_sample draws from the product of the absolute conditional marginals, which is
 * the target only for a train without sign changes; here the train approximates the square ROOT of the density (TTX_FUN_TRAINS
 * builds it), every marginal of its square is a quadratic form with a Gram matrix, and every conditional is a sum of squares:
 * non-negative whatever the signs of the cores.  u, fixed, ind, logq, val, the chunking (TTX_SAMPLE_CHUNK), the failed-sample
 * convention and the refusal of multi-process engines are ttx_sample's.  The differences:
 *   w     : NULL for all ones, or d blocks of n_k weights, finite and >= 0 (their square roots enter)
 *   gamma : finite and >= 0, the defensive term below
 *   mode  : TTX_EVAL_EXACT, TTX_EVAL_MFMA or TTX_EVAL_AUTO, as in ttx_topk: only the rows of p depend on it
 * Definition (numpy restates it: tests/sample_sq_ref.py).  Modes are 1-based, r_0 = r_d = 1.  Effective weights e_k as for
 * ttx_sample: w_k for a drawn mode, the indicator of f_k for a fixed one.  W_k = sum_i w_k(i) for a drawn mode (ascending i from
 * 0.0) and 1 for a fixed one.  Weighted prefix Gram matrices: P_0 = [1], P_k = sum_i e_k(i) G_k(:, i, :)^T P_(k-1) G_k(:, i, :).
 * They are never formed (y^T P y squares the conditioning); the call holds factors F_k of l_k = min(l_(k-1) n_k, r_k) rows with
 * F_k^T F_k = 2^(-2 s_k) P_k, F_0 = [1], from one left-to-right pass:
 *   H_k(a, i, b) = sum_a' F_(k-1)(a, a') G_k(a', i, b) (the engine's fp64 matrix-core GEMM; H_1 is a copy of G_1);
 *   F_k = the R factor (the engine's Householder QR) of the matrix whose rows (a, i) are sqrt(e_k(i)) * H_k(a, i, :); where that
 *   matrix has no more rows than columns, F_k is the matrix itself.  F_k is then multiplied by the power of two that takes its
 *   largest entry into [0.5, 1) (none where that entry is 0 or not finite); s_k is the sum of these exponents up to k.  The
 *   scaling is exact and cancels in every ratio below.
 * Draw, from the LAST mode to the first, with the state x of dtt_ijk's chain, x_(d+1) = [1].  For a drawn mode k:
 *   m(a, i) = sum_b H_k(a, i, b) x_(k+1)(b),  s(i) = sum_a m(a, i)^2.  TTX_EVAL_EXACT: both sums ascending from 0.0 with a separate
 *   multiply and add.  TTX_EVAL_MFMA: the sum over b in the order of v_mfma_f64_16x16x4_f64 (steps of four b, ascending), the sum
 *   over a ascending from 0.0 in a register (the 16 indices of a tile are the rows of the matrix operand, so no shuffle is needed);
 *   p(i) = w_k(i) * (s(i) + g_k),  g_k = gamma * prod_(j<k) W_j * 2^(-2 s_(k-1)): the defensive term in the units of F_(k-1).
 *   p >= 0 by construction, there is no absolute value.  The running sum c, t = u_k c(n_k), the search, "never an index with
 *   p = 0", the state update in TTX_EVAL_EXACT's operation sequence and logq += log(p(i_k) / c(n_k)) are ttx_sample's, in both
 *   modes: val equals ttx_ijk_batch(ind, TTX_EVAL_EXACT) bit for bit in both.  A fixed mode takes i_k = f_k and computes no p.
 * Distribution, for ANY train, signed or not: the samples follow (T(i)^2 + gamma) prod w_k(i_k) / (Z + gamma prod W_k) exactly, up
 * to rounding, over the drawn modes at the fixed indices, Z = sum_i T(i)^2 prod w.  Hence exp(logq) (Z + gamma prod W_k) =
 * (val^2 + gamma) prod w_k(i_k), and with gamma > 0 the importance weight val^2 prod w / exp(logq) is bounded by Z + gamma prod W_k.
 * Failed samples, safety, determinism: as for ttx_sample.  The sums s(i) of a chunk lie in a sheet [chunk][n_k] of the engine's work
 * space; a sample's state, logq and failure flag stay there between the per-mode launches.  No floating-point atomics; a sample
 * depends neither on its neighbours nor on the chunk; a call repeats bit for bit.  The train is not modified.
 * TTX_EVAL_AUTO takes the matrix cores from TTX_SQ_AUTO_FLOPS flops of the call on (2 sum_k npts n_k l_(k-1) r_k, drawn modes).
 * ttx_sample_sq_dev: u, ind, logq and val are pointers on the engine's device, w and fixed stay host pointers.
 * npts = 0 succeeds and launches nothing.  TTX_EINVAL: npts < 0, null u / ind with npts > 0, an unknown mode, gamma negative or not
 * finite (all before the engine is looked at); a fixed entry outside 0..n_k, a weight that is negative or not finite, ranks above
 * 128, a chunk times the largest mode above 2^28 sheet entries (before any launch); TTX_ESTATE: an engine without a train; a
 * multi-process engine is refused as by ttx_sample.
 * ttx_sample_sq_last: of the last call on this engine, the milliseconds (HIP events) of the head pass, of the rows kernels and of
 * k_sq_pick with k_sq_step (summed over modes and chunks), the flops of the rows, the failed samples and the mode that ran; any pointer may be
 * NULL.  The real-valued variant is ttx_sample_sq_real.  Open: per-sample weights, ranks above 128.  Added without a new ttx_version: look the symbols up. */
int ttx_sample_sq    (ttx_engine *h, int64_t npts, const double *u /* [npts][d] */, const double *w, const int32_t *fixed,
                      double gamma, int32_t mode, int32_t *ind, double *logq, double *val);
int ttx_sample_sq_dev(ttx_engine *h, int64_t npts, const double *u, const double *w, const int32_t *fixed,
                      double gamma, int32_t mode, int32_t *ind, double *logq, double *val);
int ttx_sample_sq_last(const ttx_engine *h, double *ms_head, double *ms_rows, double *ms_pick, double *flops, int64_t *nfailed, int32_t *mode_ran);

/* REAL-valued samples drawn from the piecewise-linear interpolant of a resident train of grid values, on the device
 * (ttcross_amd/csrc/ttx_sample_real.h): the inverse Rosenblatt transform of the interpolant that ttx_basis_batch evaluates with
 * TTX_BASIS_LINEAR, the conditional-distribution sampler of Dolgov, Anaya-Izquierdo, Fox and Scheichl (2020).  Uniforms in
 * [0, 1]^d go in; real points, the log-density of the proposal and the interpolant's value come out; no core leaves the device.
 * Modes are 1-based, G_k is core k, t_k are the n_k strictly ascending nodes of mode k, r_0 = r_d = 1.
 *   u     : npts rows of d uniforms, row-major [npts][d]; u_k draws mode k
 *   nodes : d host pointers, row k holds the n_k nodes of mode k
 *   cond  : d entries or NULL.  NaN (or cond NULL): the mode is drawn; finite: the mode is HELD at that real coordinate, on a node,
 *           between nodes or outside the node range alike (its u_k is not looked at).  A mode with n_k = 1 is always held (at its
 *           node, or at cond_k where that is finite: its hat row is (1) either way)
 *   x     : [npts][d] the samples;  cell : [npts][d] or NULL, the 1-based cell of a drawn mode, 0 for a held one;
 *   logq, val : [npts], each may be NULL
 * Definition (numpy restates it: tests/sample_real_ref.py).  phi_k(x) is the row of TTX_BASIS_LINEAR at x by the rule above
 * (ttx_basis_host is its restatement).  Effective weights e_k: for a drawn mode the trapezoid weights of the nodes, om(0) = 0.5 (t_1 -
 * t_0), om(i) = 0.5 (t_(i+1) - t_(i-1)), om(n-1) = 0.5 (t_(n-1) - t_(n-2)); for a held mode phi_k(cond_k).  Prefix vectors l_0 = [1],
 * l_k = l_(k-1) M_k with M_k = sum_i e_k(i) G_k(:, i, :), formed by the kernels of ttx_marginals in their summation order, as for
 * ttx_sample.  Head table of a drawn mode: H_k(i, b) = sum_a l_(k-1)(a) G_k(a, i, b), ttx_sample's with weights of 1.0.
 * Draw.  x_(d+1) = [1]; for k = d .. 1 of a drawn mode, with h_j = t_(j+1) - t_j:
 *   p(i) = |sum_b H_k(i, b) x_(k+1)(b)|  (ascending b from 0.0, separate multiply and add), i = 0 .. n-1: the nodal conditional
 *   A(j) = (0.5 * (p(j) + p(j+1))) * h_j, j = 0 .. n-2: the mass of cell j under the interpolated conditional
 *   C    = the inclusive running sum of A in ttx_sample's association order (blocks of 64, six doubling steps inside a block)
 *   T = u_k * C(n-2);  j = the smallest cell with A(j) > 0 and T < C(j).  If there is none, or u_k >= 1: the largest cell with
 *   A > 0 and lambda = 1.  Otherwise s = min(max(T - C(j-1), 0), A(j)) (C(-1) = 0), s' = s / h_j, D = p(j+1) - p(j),
 *   disc = max(p(j) * p(j) + (2 * D) * s', 0), den = p(j) + sqrt(disc), lambda = den > 0 ? (2 * s') / den : 0, clamped to [0, 1]:
 *   the root of p(j) l + D l^2 / 2 = s' in the form that has no cancellation.  p(j), p(j+1) and s' are first multiplied by the
 *   power of two that takes max(p(j), p(j+1)) into [0.5, 1): exact, and the same bits wherever p(j)^2 neither under- nor overflows.
 *   x_k = t_j + lambda * h_j, clamped to [t_j, t_(j+1)];  cell = j + 1.
 * Chain step, all modes.  phi = phi_k(x_k) is formed again from the rounded x_k by the basis rule (for a held mode x_k = cond_k); where
 * x_k rounded onto the node t_(j+1) it therefore names cell j + 1.  With i, i + 1 the at most two nonzero entries (i the rule's cell,
 * at most n_k - 2):  z(a) = (0.0 + phi_i * tau_i(a)) + phi_(i+1) * tau_(i+1)(a),  tau_i(a) = sum_b G_k(a, i, b) x_(k+1)(b) in the
 * operation sequence of TTX_EVAL_EXACT;  x_k-state = z.  For a finite train this is ttx_basis_batch's TTX_EVAL_EXACT chain, whose
 * other terms are products with 0.0.  The log term of a drawn mode is log((phi_i * p(i) + phi_(i+1) * p(i+1)) / C(n-2)).
 * Outputs: x; cell; logq = the sum of the log terms over the drawn modes, k = d .. 1: the log of the proposal's density at x with
 * respect to Lebesgue measure on the drawn modes (-inf where that density vanishes at x); val = z(1) after mode 1, the interpolant
 * at x: equal to ttx_basis_batch(x, TTX_BASIS_LINEAR on nodes, TTX_EVAL_EXACT) element for element (up to the sign of a zero).
 * Distribution: for a train without sign changes the samples follow the multilinear interpolant f(x) / Z exactly, up to rounding,
 * and exp(logq) = val / Z with Z = ttx_quad with the trapezoid weights (1.0 for a mode of one node; for held modes their hat
 * rows).  For a signed train they follow the product of the interpolated ABSOLUTE nodal conditionals; exp(logq) is the proposal
 * density to reweight with.
 * Failed samples: C(n-2) is 0, NaN or Inf at some mode, or the u_k of a drawn mode is NaN or negative (-0.0 counts as 0).  The whole
 * row of x is NaN, cell is 0, logq NaN and val 0.0; the sample is counted (ttx_sample_real_last); the others are untouched.
 * Safety, as for ttx_sample: a cell index is formed from lane numbers, never from a value; x_k is clamped into its cell before the
 * hat row is looked up, whose cell is j or j + 1, capped at n_k - 2; the cell of a held mode is found on the host.  Whatever cores,
 * nodes and u hold, no read leaves its table.  Arithmetic is plain double without a running exponent.
 * A sample depends neither on its neighbours nor on the chunk (TTX_SAMPLE_CHUNK); a call repeats bit for bit.  The train is not
 * modified; the work space is the engine's own.  ttx_sample_real_dev: u, x, cell, logq and val are pointers on the engine's
 * device, nodes and cond stay host pointers; it enqueues on the engine's stream and synchronises before it returns.
 * npts = 0 succeeds and launches nothing.  TTX_EINVAL: npts < 0, null u / x / nodes with npts > 0 (before the engine is looked
 * at); a node row that is missing, not finite or not strictly ascending, cond_k = +-Inf (before any device call); ranks above 128.
 * TTX_ESTATE: an engine without a train; a multi-process engine is refused as by ttx_sample.
 * ttx_sample_real_last: as ttx_sample_last, for k_sm_head and k_sr_draw of the last ttx_sample_real on this engine.
 * For a signed train ttx_sample_sq_real draws from the squared interpolant.  Open: a direct COS-basis sampler (root finding on a density that may go negative), an MFMA
 * path for the rows of p, extra per-mode weights, ranks above 128.  Added without a new ttx_version: look the symbols up. */
int ttx_sample_real    (ttx_engine *h, int64_t npts, const double *u /* [npts][d] */, const double *const *nodes /* [d] host rows of n_k */,
                        const double *cond /* [d] or NULL */, double *x /* [npts][d] */, int32_t *cell /* [npts][d] or NULL */, double *logq, double *val);
int ttx_sample_real_dev(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double *x, int32_t *cell, double *logq, double *val);
int ttx_sample_real_last(const ttx_engine *h, double *ms_head, double *bytes_head, double *ms_draw, int64_t *nfailed);

/* REAL-valued samples drawn from the SQUARE of the interpolant of the resident train, on the device
 * (ttcross_amd/csrc/ttx_sample_sq_real.h): ttx_sample_sq's squared-density sampler (SIRT: Cui and Dolgov, 2022) on the continuous
 * domain of ttx_sample_real.  The resident train holds grid values of g at the nodes t_k; g(x) is its piecewise-multilinear
 * interpolant, what ttx_basis_batch evaluates with TTX_BASIS_LINEAR and TTX_EVAL_EXACT.  The call draws from
 *   (g(x)^2 + gamma) / (Z + gamma V)
 * over the drawn modes: Z is the integral of g^2 over the box of the drawn modes at the held coordinates, V the product of
 * t_(n-1) - t_0 over the drawn modes.  Every conditional is a sum of squares, so this holds for ANY train, signed or not.
 * u, nodes, cond, x, cell, logq, val and the held-mode rules (a finite cond_k holds the mode at that real coordinate, n_k = 1 is
 * always held) are ttx_sample_real's; gamma and mode are ttx_sample_sq's.
 * Definition (numpy restates it: tests/sample_sq_real_ref.py).  h_i = t_(i+1) - t_i.
 * Mass factors, on the host.  For a drawn mode the hat functions' mass matrix M_k is tridiagonal: M(i, i) = (h_(i-1) + h_i) / 3.0
 * with one term at each end, M(i, i+1) = h_i / 6.0.  Its Cholesky factor M_k = U_k^T U_k is upper bidiagonal:
 *   dg(0) = sqrt(M(0,0)),  sp(i) = M(i,i+1) / dg(i),  dg(i+1) = sqrt(M(i+1,i+1) - sp(i) * sp(i)),  sp(n-1) = 0,
 * in plain double with separate operations.  For a held mode dg and sp are zero except dg(ci) = phi0 and sp(ci) = phi1, the hat row
 * of cond_k by ttx_basis_host's rule (ci its cell).
 * Head pass: ttx_sample_sq's, with the rows handed to the QR generalised to dg(i) H_k(a, i, :) + sp(i) H_k(a, i+1, :) (the last
 * index has the first term only).  F_k, the power-of-two scaling and s_k are unchanged;
 *   g_k = gamma * prod_(j<k) L_j * 2^(-2 s_(k-1)),  L_j = t_(n-1) - t_0 for a drawn mode and 1 for a held one.
 * Draw, from the LAST mode to the first, with the state x of dtt_ijk's chain, x_(d+1) = [1].  For a drawn mode k:
 *   m(a, i) = sum_b H_k(a, i, b) x_(k+1)(b),  s(i) = sum_a m(a, i)^2 (i = 0 .. n-1),  c(j) = sum_a m(a, j) m(a, j+1) (j = 0 .. n-2).
 *   TTX_EVAL_EXACT: all sums ascending from 0.0 with a separate multiply and add.  TTX_EVAL_MFMA: the sum over b in the order of
 *   v_mfma_f64_16x16x4_f64, the sums over a ascending from 0.0 in a register.
 *   lim = sqrt(s(j)) * sqrt(s(j+1)); c(j) is clamped into [-lim, lim] (a NaN passes through): the conditional cannot go negative
 *   inside a cell.  q0 = s(j) + g_k, qm = c(j) + g_k, q1 = s(j+1) + g_k: the density along the cell is
 *   q(l) = q0 (1-l)^2 + 2 qm l (1-l) + q1 l^2.  Cell mass A(j) = (((q0 + qm) + q1) / 3.0) * h_j.
 *   The running sum C, T = u_k * C(n-2), the search "smallest cell with A > 0 and T < C", the rule "u >= 1 or none: the largest
 *   cell with A > 0, lambda = 1" and s = min(max(T - C(j-1), 0), A(j)) are ttx_sample_real's.  Inside the cell lambda in [0, 1]
 *   solves Q(l) = s / h_j, Q the cubic with Bernstein coefficients 0, q0/3, (q0 + qm)/3, (q0 + qm + q1)/3, by sqr_invert: the four
 *   numbers are scaled by the power of two that takes max(q0, |qm|, q1) into [0.5, 1); then, from l = 0.5 on the bracket [0, 1], at
 *   most 64 times: f = l * (q0 + l * ((qm - q0) + l * (((q0 - 2.0 * qm) + q1) / 3.0))) - s'; f > 0 lowers the upper end to l,
 *   otherwise the lower end rises to l; the Newton step l - f / q(l), q(l) = q0 + l * (2.0 * (qm - q0) + l * ((q0 - 2.0 * qm) + q1)),
 *   is taken if q(l) > 0 and it lies strictly inside the bracket, else the bracket's midpoint; it ends when l no longer changes.
 *   s' <= 0 gives 0, s' >= Q(1) gives 1, anything that is not a number 0.  It holds where q touches zero inside the cell (a sign
 *   change of g: qm = -sqrt(q0 q1), Q is flat).
 *   x_k, its clamp into the cell, the cell of the rounded x_k and the hat values f0, f1 formed again from the rounded x_k are
 *   ttx_sample_real's.  Log term, with i the hat cell: log(max((((f0*f0)*s(i) + ((2.0*f0)*f1)*c(i)) + (f1*f1)*s(i+1)) + g_k, 0) / C(n-2)).
 * Chain step, all modes: ttx_sample_real's.  val equals ttx_basis_batch(x, TTX_BASIS_LINEAR on nodes, TTX_EVAL_EXACT) element for
 * element in both modes; logq is the log of the proposal's density at x with respect to Lebesgue measure on the drawn modes, and
 * for any train exp(logq) (Z + gamma V) = val^2 + gamma up to rounding: with gamma > 0 the importance weight val^2 / exp(logq)
 * is bounded by Z + gamma V.
 * Failed samples (row of NaN in x, cell 0, logq NaN, val 0.0, counted), safety, determinism and chunking (TTX_SAMPLE_CHUNK): as
 * for ttx_sample_real and ttx_sample_sq.  The sums s and c of a chunk lie in two sheets [chunk][n_k] of the engine's work space; a
 * sample's state, logq, failure flag and hat values stay there between the per-mode launches.  Every index comes from lane
 * numbers, never from a value; the hat cell is range-checked again where the chain step reads it.  The train is not modified.
 * TTX_EVAL_AUTO uses ttx_sample_sq's TTX_SQ_AUTO_FLOPS: on the D_64 train the two modes of this entry part in the same bracket, between
 * 1.9e9 flops per call (a tie) and 1.9e10 (the matrix cores 2.5 times faster); profiles/sample_sq_real_mi355x.txt.
 * ttx_sample_sq_real_dev: u, x, cell, logq and val are pointers on the engine's device, nodes and cond stay host pointers.
 * npts = 0 succeeds and launches nothing.  TTX_EINVAL: npts < 0, null u / x / nodes with npts > 0, an unknown mode, gamma negative
 * or not finite (all before the engine is looked at); a node row that is missing, not finite or not strictly ascending, cond_k =
 * +-Inf, ranks above 128, two sheets of a chunk times the largest mode above 2^28 entries (before any launch).  TTX_ESTATE: an
 * engine without a train; a multi-process engine is refused as by ttx_sample.
 * ttx_sample_sq_real_last: as ttx_sample_sq_last, for the head pass, the rows kernels and k_sqr_pick with k_sqr_step.
 * Open: per-sample weights, ranks above 128.  Added without a new ttx_version: look the symbols up. */
int ttx_sample_sq_real    (ttx_engine *h, int64_t npts, const double *u /* [npts][d] */, const double *const *nodes /* [d] host rows of n_k */,
                           const double *cond /* [d] or NULL */, double gamma, int32_t mode, double *x /* [npts][d] */, int32_t *cell /* [npts][d] or NULL */,
                           double *logq, double *val);
int ttx_sample_sq_real_dev(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *x,
                           int32_t *cell, double *logq, double *val);
int ttx_sample_sq_real_last(const ttx_engine *h, double *ms_head, double *ms_rows, double *ms_pick, double *flops, int64_t *nfailed, int32_t *mode_ran);

/* The way back: the FORWARD Rosenblatt map of the squared interpolant, x -> u, on the device (k_sqr_cdf,
 * ttcross_amd/csrc/ttx_sample_sq_real.h).  ttx_sample_sq_real takes uniforms u to points x; this entry takes points x the sampler
 * did not draw to the uniforms u that map to them, with logq, the log of the proposal's density (g(x)^2 + gamma) / (Z + gamma V)
 * at x, and val = g(x): the acceptance ratio of an independence Metropolis step, logq for mixtures over several trains, the
 * probability integral transform of held-out data, the forward half of a layered transport (DIRT: Cui and Dolgov, 2022).
 * nodes, cond, gamma, mode, the held-mode rules, the chunking (TTX_SAMPLE_CHUNK), TTX_EVAL_AUTO's threshold (TTX_SQ_AUTO_FLOPS) and
 * the sheet limit are ttx_sample_sq_real's.  x is [npts][d] where the sampler has u; u is [npts][d] where it has x.
 * Definition (numpy restates it: tests/rosenblatt_ref.py).  The mass factors, the head pass, g_k, the rows s(i) and c(j), the clamp
 * of c, q0, qm, q1 and A(j) are those of ttx_sample_sq_real, word for word.  The modes are walked k = d .. 1 with the state
 * x_(d+1) = [1].
 * A held mode: x[:, k] is not looked at, u_k = 0.0 and cell = 0; the chain step uses the host-made hat row of cond_k, as in the
 * sampler.  u_k is 0.0 and not NaN, so that a failed row stays recognisable by its first entry.
 * A drawn mode: ci = sr_hat_cell(t, n, x_k), TTX_BASIS_LINEAR's cell: the last node with t_ci <= x_k, at most n - 2.
 *   f1 = (x_k - t_ci) / (t_(ci+1) - t_ci), f0 = 1.0 - f1: the sampler's expressions for its rounded x_k.
 *   C is the inclusive running sum of A in the sampler's association: lanes along j in rounds of 64, inside a round added in
 *   ascending distance 1, 2, .. 32, the carry from round to round through lane 63.  C(n-2) is the total, C(-1) = 0.
 *   The mass inside the cell is min(max(h_ci * sqr_cdf(q0, qm, q1, f1), 0), A(ci)) with the q of cell ci.  sqr_cdf scales q0, qm, q1
 *   by sqr_invert's power of two, evaluates the Horner form the inversion iterates on,
 *     l * (q0 + l * ((qm - q0) + l * (((q0 - 2.0 * qm) + q1) / 3.0))),
 *   returns 0 for l <= 0 and ((q0 + qm) + q1) / 3.0 for l >= 1, and scales back by ldexp; anything that is not a number gives 0.
 *   u_k = (C(ci-1) + mass inside) / C(n-2), clamped into [0, 1];  cell = ci + 1.
 *   Log term: the sampler's, on ci, f0, f1: log(max((((f0*f0)*s(ci) + ((2.0*f0)*f1)*c(ci)) + (f1*f1)*s(ci+1)) + g_k, 0) / C(n-2)).
 *   A cell without mass is no failure: the term is -inf and u_k is the running sum before it.  (Inside such a cell g is 0 along the
 *   whole cell, so the state after the chain step is 0: in a mode walked before the last the next mode finds C(n-2) = 0 and the point
 *   fails there, unless gamma > 0.  Mode 1, walked last, shows the -inf.)
 * Chain step, all modes: the sampler's (k_sqr_step, unchanged).  val = z(1) after mode 1, ttx_basis_batch(x, TTX_BASIS_LINEAR on
 * nodes, TTX_EVAL_EXACT) element for element.  The sampler forms cell, hat values and log term from its ROUNDED x, so at the
 * sampler's own x, in the same mode, logq and val repeat bit for bit; cell is the sampler's, or one more exactly where x sits on
 * the right node of its cell; u comes back within the rounding of the cubic and of the sums (tests/rosenblatt_ref.py derives it).
 * A failed point: a drawn coordinate is NaN or lies outside [t_0, t_(n-1)], or C(n-2) is 0, NaN or Inf at some mode.  The
 * convention is the samplers': the whole row of u is NaN, cell 0, logq NaN, val 0.0, and the point is counted.  Safety,
 * determinism and work space are the sampler's: every index comes from lane numbers or from a count of nodes, the cell is
 * range-checked where it is read, no read leaves its table whatever x holds; a call repeats bit for bit.  The train is not modified.
 * ttx_rosenblatt_sq_real_dev: x, u, cell, logq and val are pointers on the engine's device, nodes and cond stay host pointers.
 * npts = 0 succeeds and launches nothing.  TTX_EINVAL: npts < 0, null x / u / nodes with npts > 0, an unknown mode, gamma negative
 * or not finite (all before the engine is looked at); a node row that is missing, not finite or not strictly ascending, cond_k =
 * +-Inf, ranks above 128, two sheets of a chunk times the largest mode above 2^28 entries (before any launch).  TTX_ESTATE: an
 * engine without a train; a multi-process engine is refused as by ttx_sample.
 * ttx_rosenblatt_sq_real_last: as ttx_sample_sq_real_last, in a slot of its own (the sampler's figures stay), for the head pass, the
 * rows kernels and k_sqr_cdf with k_sqr_step.
 * Open: points outside the box as density 0 (logq = -inf) rather than as failures, per-point weights, ranks above 128.  Added
 * without a new ttx_version: look the symbols up. */
int ttx_rosenblatt_sq_real    (ttx_engine *h, int64_t npts, const double *x /* [npts][d] */, const double *const *nodes /* [d] host rows of n_k */,
                               const double *cond /* [d] or NULL */, double gamma, int32_t mode, double *u /* [npts][d] */, int32_t *cell /* [npts][d] or NULL */,
                               double *logq, double *val);
int ttx_rosenblatt_sq_real_dev(ttx_engine *h, int64_t npts, const double *x, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *u,
                               int32_t *cell, double *logq, double *val);
int ttx_rosenblatt_sq_real_last(const ttx_engine *h, double *ms_head, double *ms_rows, double *ms_cdf, double *flops, int64_t *nfailed, int32_t *mode_ran);

/* The largest elements of the resident train by a beam search along the train, on the device (ttcross_amd/csrc/ttx_topk.h), with
 * an upper bound on everything the search discarded.  Modes are 1-based, G_k is core k, r_0 = r_d = 1.
 *   K     : rows wanted, 1 .. 4096, and K max n_k <= 2^24 (the score sheet of one mode is kept in work space)
 *   which : TTX_TOPK_ABS, TTX_TOPK_MAX, TTX_TOPK_MIN: how the returned rows are ORDERED.  The search itself always ranks by absolute size
 *   fixed : d entries, 0 = the mode is searched, f in 1..n_k = the mode is held at index f; NULL = all searched (as ttx_sample's)
 *   mode  : TTX_EVAL_EXACT scores by plain loops (the checker), TTX_EVAL_MFMA on the fp64 matrix cores, TTX_EVAL_AUTO lets the
 *           engine choose by the flops of the call (ttx_topk_last tells what ran)
 *   ind   : [K][d], 1-based, the layout ttx_ijk_batch reads;  val : [K];  nfound, bound : one number each
 * Definition.  I_k is 1..n_k for a searched mode and {f_k} for a fixed one.  Prefix Gram matrices: P_0 = [1],
 *   P_k = sum over i in I_k of G_k(:, i, :)^T P_(k-1) G_k(:, i, :)   (r_k x r_k; ascending i).
 * For a vector y of length r_(k-1), y^T P_(k-1) y is the squared 2-norm of the slice of the tensor over all prefixes in
 * I_1 x .. x I_(k-1) whose suffix has the running vector y, whether or not the train was orthogonalised.
 * Search from the LAST mode to the first, so the running state is dtt_ijk's own chain.  C_(d+1) holds one candidate, the empty
 * suffix with x = [1].  For k = d .. 1 every candidate c of C_(k+1), in its order, and every i of I_k, ascending, give
 *   y = G_k(:, i, :) x_c   and the score   s(c, i) = sqrt(max(0, y^T P_(k-1) y))   at the flat position c |I_k| + i.
 * C_k is the K pairs with the largest score (all pairs if there are no more than K), kept in ascending flat position; ties go to the
 * smaller flat position, a NaN score ranks below every number, +Inf first.  bound_k is the largest score among the pairs not
 * kept, 0 if all were kept.  The x of a kept pair is formed by the operation sequence of ttx_ijk_batch's TTX_EVAL_EXACT (sums from
 * 0.0 over ascending b, separate multiply and add, two rows per lane above rank 64; x_d is a copy of G_d(:, i_d, 1)) -- in BOTH
 * modes: only the scores come from the matrix cores.  Hence val = x_1(1) equals ttx_ijk_batch(ind, TTX_EVAL_EXACT) bit for bit.
 * At k = 1 the score is |y| (r_0 = 1, P_0 = [1]); under TTX_EVAL_EXACT y is formed in the chain's own order, so the score is |val|.
 * TTX_EVAL_EXACT sums z = P y over ascending columns from 0.0 and adds y(a) z(a) per lane over a = lane, lane + 64 and across the
 * lanes in xor steps 32 .. 1; TTX_EVAL_MFMA takes v_mfma_f64_16x16x4_f64's own order.  The two agree to rounding.
 * Outputs.  nfound = |C_1| = min(K, prod |I_k|).  The first nfound rows of ind / val are ordered by `which` (ABS: |val| descending,
 * MAX: val descending, MIN: val ascending; a NaN value after every number), ties by the lexicographically smaller index row, so
 * the order does not depend on the internal candidate order.  The remaining rows are zeros and 0.0.  bound = max_k bound_k; if any
 * score of the call was NaN, bound is NaN.
 * Guarantee.  |T(prefix, suffix)| is at most the 2-norm of the slice over the prefixes, so every element of the tensor at the
 * fixed indices that is not among the returned ones has |T(i)| <= bound, up to the rounding of the scores.  Hence bound <= |val|
 * of the last row (ordered by TTX_TOPK_ABS) proves that the rows are the true top nfound by absolute size, and bound <= |val[0]|
 * proves the maximum alone.  On a peaked, density-like train K = 1 may already prove the maximum; on a random train the bound
 * proves nothing until K approaches an exhaustive search.  The rounding of the Gram route grows with the conditioning of P: a
 * score is the root of a difference of large terms when P is ill-conditioned.  After ttx_ort P is a multiple of the identity to
 * rounding and the scores are as accurate as the chain; nothing in the call requires ttx_ort.
 * Safety: a selection compares 64-bit keys (the score's bit pattern + 1, NaN = 0), every index is formed from positions and counts
 * and a stored position is range-checked where it is read: whatever the cores hold (NaN, Inf) every index written lies in range
 * and no read leaves its table.  No floating-point atomics, no sum whose order depends on the grid: a call repeats bit for bit
 * in either mode (integer atomics count keys and take the maximum key).
 * TTX_EINVAL: null nfound / ind / val / bound, K outside 1..4096, unknown which or mode (all before the engine is looked at); a
 * fixed entry outside 0..n_k, K max n_k > 2^24, ranks above 128 (before any launch).  TTX_ESTATE: an engine without a train; a
 * multi-process engine is refused as by ttx_ijk (a replica, ttx_replicate, is accepted).  The train and the engine's other work
 * space are not modified.  Everything is enqueued on the engine's stream; the call synchronises after every mode (the timers) and
 * before it returns.
 * ttx_topk_last: of the last call on this engine, the milliseconds (HIP events, summed over the modes) of the Gram chain, of the
 * scoring launches and of the selection launches (radix select, compaction and the advance of the kept pairs),
 * flops = 2 sum_k |C_(k+1)| |I_k| r_(k-1) (r_k + r_(k-1)), and the mode that ran (-1: none yet).  Any pointer may be NULL.
 * Added without a new ttx_version: look the symbols up. */
#define TTX_TOPK_ABS 0   /* rank the results by |T(i)|, largest first */
#define TTX_TOPK_MAX 1   /* by T(i), largest first  */
#define TTX_TOPK_MIN 2   /* by T(i), smallest first */
int ttx_topk(ttx_engine *h, int32_t K, int32_t which, const int32_t *fixed /* [d] or NULL */, int32_t mode,
             int32_t *nfound, int32_t *ind /* [K][d], 1-based */, double *val /* [K] */, double *bound);
int ttx_topk_last(const ttx_engine *h, double *ms_gram, double *ms_score, double *ms_select, double *flops, int32_t *mode_ran);

/* The finalised train of a MULTI-PROCESS job gathered onto EVERY process as a new single-process engine (same integrand, ranks,
 * RNG position; *out is owned by the caller: ttx_destroy).  Collective over the job's transport (each process contributes the
 * cores it holds; the others arrive by a SUM all-reduce into zero-filled slots, which is exact).  The reference's dtt_accchk,
 * norm, dot_product, ort, svd and dtt_write expect a type(dtt) with all cores (lib/tt.f90; lib/dmrgg.f90:1081-1166). */
int ttx_replicate(ttx_engine *h, ttx_engine **out);

/* Tensor trains that do not come from a sweep.
 * ttx_from_tt : upload a train given as compact column-major cores (d blocks r(k-1)*n(k)*r(k), concatenated) and make
 *               it the resident train of a new single-process engine (the reference: plain assignment into arg%u(k)%p);
 *               all of ttx_get_*, ttx_quad, ttx_zquad and the tt_lib utilities work on it; ttx_run / ttx_accchk do not
 *               (no integrand).  ranks must be <= 128.
 * ttx_write   : dtt_write (lib/ttio.f90:29-108), the reference's raw stream file: 128-byte header `tthead`
 *               (lib/ttio.f90:10-17), l, m, n(l:m), r(l-1:m) as int32, all cores as float64; l = 1.
 * ttx_read    : dtt_read (lib/ttio.f90:196-297) of such a file into a new engine (checks 'TT' and version 1).
 * ttx_get_modes: arg%m and arg%n(1:m) of an engine (n may be NULL). */
int ttx_from_tt(ttx_engine **out, int32_t d, const int32_t *n, const int32_t *r, const double *cores, int32_t device);
int ttx_write(const ttx_engine *h, const char *path);
int ttx_read(ttx_engine **out, const char *path, int32_t device);
int ttx_get_modes(const ttx_engine *h, int32_t *d, int32_t *n);
/* save_dtt_to_hdf5 (lib/utils.f90:8-57): group "TT", datasets "modes", "ranks" (native int) and "core_k", k = 0..m-1, with
 * the Fortran shape (r(k-1), n(k), r(k)); ttx_read_hdf5 loads such a file into a new engine (the reference has no
 * reader; this one exists for round trips and checkpoints).  libhdf5.so is resolved at run time (dlopen): without it both
 * return TTX_EINVAL with a message. */
int ttx_write_hdf5(const ttx_engine *h, const char *path);
int ttx_read_hdf5(ttx_engine **out, const char *path, int32_t device);

/* profiling: with on != 0 the next ttx_run brackets every kernel launch with HIP events on the engine's
 * stream; ttx_kernel_stats then reports, per kernel kind, launches and total milliseconds. */
#define TTX_K_LOTTERY 0
#define TTX_K_HALFSTEP 1   /* fiber evaluation + residual + argmax (the north star's "maxvol" kernel) */
#define TTX_K_ACCEPT 2
#define TTX_K_EXCHANGE 3
#define TTX_K_QUAD 4
#define TTX_K_OTHER 5
#define TTX_K_NKINDS 6
int ttx_set_profile(ttx_engine *h, int on);
/* which implementation of the sweep this engine uses (TTX_SWEEP=auto|chain|fused|cluster chooses at ttx_create):
 * 0 multi-kernel chain (k_lottery / k_halfstep / k_accept per bond), 1 one workgroup per bond group for the whole
 * sweep (k_sweep_fused), 2 a cluster of workgroups per bond group for the whole sweep (k_sweep_cluster) */
int ttx_sweep_path(const ttx_engine *h);
/* the kernels this engine would launch now, one line per stage, as NUL-terminated text in buf (cap bytes; TTX_EINVAL if too small).
 * Read-only, usable right after ttx_create; a fallback of ttx_run changes it.  Kernels by their source names with the template
 * arguments that select behaviour; "-": the stage launches nothing.
 *     path: chain|fused|cluster
 *     tables: <kernel or ->
 *     lottery: <kernel>                    or  <kernel> + <candidate evaluator> + <kernel>   (-: full pivoting draws none)
 *     halfstep: <kernel>[<=N], <kernel>[<=M], <kernel>    (a tier is taken while the sweep's units * groups are at most its bound)
 *     fullpiv: plain|mfma|columns          (pivoting -1 only: every column at once, the dense MFMA step, one column per host pass)
 * The last lines describe the multi-kernel chain also where a whole-sweep kernel is in use: they are what a fallback runs. */
int ttx_plan_describe(const ttx_engine *h, char *buf, int64_t cap);
/* the integrand evaluator inside the cluster kernel (one instantiation of k_sweep_cluster each): 0 the engine is not on the cluster
 * path, 1 exact chains with predicated remainders (any node values; TTX_CL_PAD=0 asks for it), 2 exact chains over rows padded to
 * whole chunks of 8 with neutral elements (the default where every Ising node lies in [0,1]; same bits), 3 the closed form of
 * TTX_ARITH_FAST */
int ttx_cluster_eval(const ttx_engine *h);
/* the arithmetic this engine evaluates its integrand with (TTX_ARITH_*): FAST only where ttx_config.arith / TTX_ARITH asked for
 * it AND the integrand has a re-associated evaluator (Ising D/E with all nodes in [0,1], mvn); everything else runs exact */
int ttx_arith(const ttx_engine *h);
/* runs of this engine that were replayed on the multi-kernel chain because a wait inside the cluster kernel timed out
 * (its workgroups must all be resident at once; the launch is cooperative and gated by the occupancy calculator, so this
 * is a safety net: after a fallback the engine stays on the chain path; results are identical on every path) */
int ttx_cluster_fallbacks(const ttx_engine *h);
/* the entry of a cluster launch: out[0] the forms in force as bits -- 1 the generator's jump powers from a table (TTX_CL_POWTAB=0
 * turns it off), 2 the generator word carried from the launch before (TTX_CL_WORD=0), 4 the sorted pivot lists carried from the
 * launch before (TTX_CL_LISTS=0) -- and, of the last run's launches of local group 0, out[1] those that took the carried lists and
 * out[2] those that took the carried word.  All 0 off the cluster path.  Results are identical in every form. */
int ttx_cluster_entry(const ttx_engine *h, int64_t out[3]);
/* the stretch between two sweeps of the pipelined cluster loop, the forms in force: out[0] 1 the tail launch's event is the launch's
 * own completion signal, 0 it is recorded behind the launch (TTX_TAIL_EVENT=marker asks for that; the engine also goes back to it
 * for the rest of its life once the runtime refuses the extended launch, counted in out[1]); out[2] the boundary blocks of the
 * exchange request their header words together and evaluate the corner of Ising C over staged values (TTX_TAIL_LEAN=0 turns it
 * off); out[3] the cluster kernel's exit packs the left-going message on workgroup 1 (TTX_CL_PACK2=0).  Results are identical in
 * every form. */
int ttx_sweep_gap(const ttx_engine *h, int32_t out[4]);
/* runs of this engine that were repeated without the wave teams / the wave relay of the Ising D/E half-step because a launch
 * reported a fault (more units than the grid the host sized, a broken hand-over); results are identical on every path */
int ttx_det_fallbacks(const ttx_engine *h);
int ttx_fun_id(const ttx_engine *h);                /* TTX_FUN_* the engine was created with (0: a loaded train without integrand) */
int64_t ttx_resid_halfsteps(const ttx_engine *h);   /* rook half-steps of the last run that computed a residual + arg-max (all groups) */
int ttx_kernel_stats(const ttx_engine *h, int64_t launches[TTX_K_NKINDS], double ms[TTX_K_NKINDS], double bytes[TTX_K_NKINDS]);

/* ---- kernel-level entry points used by the parity tests (host buffers in, host buffers out) ---- */

/* K2: residual + first-argmax of one rook half-step (lib/dmrgg.f90:537-546 / 570-579):
 * b = a - F*x in netlib dgemv order, F = m x r column-major (ld m); returns 0-based argmax and b[argmax]. */
int ttx_k_residual_argmax(int32_t device, int32_t m, int32_t r, const double *a, const double *F, const double *x,
                          double *b_out, int32_t *imax, double *bmax);
/* K2 streaming benchmark: the same residual + arg-max kernel on a synthetic m x r factor resident in HBM
 * (m*r*8 bytes, generated on the device); returns the average kernel time over `iters` launches measured with
 * HIP events, and the algorithmic bytes 8*(m*r + r + 2*m) one launch moves. */
int ttx_k_residual_bench(int32_t device, int64_t m, int32_t r, int32_t iters, double *avg_ms, double *bytes);
/* K1: batch integrand evaluation, ind = npts x d (row-major, 1-based indices); fun_id ISING, STDNORM, MVN or COSCOEFF
 * (anything else, and a COSCOEFF aux that ttx_create would refuse, is TTX_EINVAL before any device call; a loaded integrand,
 * TTX_FUN_DEVICE, belongs to an engine: ttx_eval_device) */
int ttx_k_eval(int32_t device, int32_t fun_id, int32_t d, const int32_t *n, const double *par, int32_t npar,
               const double *aux, int32_t naux, int64_t npts, const int32_t *ind, double *out);
/* the same with the arithmetic named (TTX_ARITH_FAST: the re-associated one-thread evaluator of ttx_fast.h; Ising D/E, nodes in [0,1]) */
int ttx_k_eval_arith(int32_t device, int32_t fun_id, int32_t d, const int32_t *n, const double *par, int32_t npar,
                     const double *aux, int32_t naux, int64_t npts, const int32_t *ind, double *out, int32_t arith);
/* lottery2 (lib/rnd.f90:105-126) with unit weights except zero at the listed 1-based positions */
int ttx_k_lottery(int32_t device, int32_t npnt, int32_t m, int32_t n, int32_t nz, const int32_t *zcol,
                  const int32_t *zrow, uint64_t rngpos, int32_t *points /* [2*npnt] */);
/* The table evaluators of TTX_ARITH=fast (ttx_fast.h) on one hand-made bond p of a d-dimensional problem with n nodes per mode,
 * element by element (tests/test_gpu_fast_elements.py).  fun_id ISING (D or E, nodes in [0,1]; par = nodes[n], weights[n], id) or
 * MVN (par = nodes, aux as ttx_create takes it).  Lidx [rL][p-1] / Ridx [rR][d-p-1]: the pivots' 1-based mode indices.  chain 0:
 * every table entry from scratch; 1: grown one dimension at a time towards the bond by the child update.  cap: rows of the decay
 * tables the lottery route finds in LDS (0..d+1).  pts [npts][d]: full multi-indices for the one-wave point evaluator.
 * Out, with FD = d+1, RM = max(rL, rR): near, dv [2][FD][RM] (side, row, pivot; near = decay vector / mvn: Y), piv [2][8][RM]
 * (rows FP_T .. FP_N), the block [rL][n][n][rR] by the lottery route (lot), by column fibers (colf) and by row fibers (rowf),
 * nfar [n*rR + rL*n]: far-vector entries above the cut per column fiber (k + n*q), then per row fiber (i + rL*j), pnt [npts]. */
int ttx_k_fast_block(int32_t device, int32_t fun_id, int32_t d, int32_t n, const double *par, int32_t npar, const double *aux, int32_t naux,
                     int32_t p, int32_t rL, const int32_t *Lidx, int32_t rR, const int32_t *Ridx, int32_t cap, int32_t chain,
                     int64_t npts, const int32_t *pts, double *near, double *dv, double *piv, double *lot, double *colf, double *rowf,
                     double *nfar, double *pnt);
/* The same tables as a fast-mode run left them (read-only, after ttx_run): side 0 = left pivots of `bond` (first-1 .. last of the
 * local group), side 1 = right pivots of `bond` (first .. last+1).  info = {r: live pivots of the bond, first, last}; with idx = NULL
 * only first and last are set.  Compact copies of the live columns: idx [d][r] (row x = x-th dimension of the multi-index: dims 1..
 * on the left, bond+1.. on the right), near / dv [d+1][r], piv [8][r]; cols = columns the buffers hold (maxrank is enough).  dv is
 * written for mvn only. */
int ttx_fast_tables(const ttx_engine *h, int32_t group, int32_t side, int32_t bond, int32_t cols, int32_t *info, int32_t *idx, double *near,
                    double *dv, double *piv);

/* exp() of the integrands (test_crs_stdnorm.f90:168, lib/mvn_pdf.f90:82): the device code restates the run-time
 * library's algorithm operation for operation (ttx_exp.h).  ttx_k_exp evaluates it on the device, ttx_exp_host the same
 * source on the host (needs no GPU) -- both exist so that tests can pin it against libm bit for bit. */
int ttx_k_exp(int32_t device, int64_t n, const double *x, double *out);
int ttx_exp_host(int64_t n, const double *x, double *out);

/* latency probe (bench.py's latency model of the sweep kernels): ns per dependent fp64 multiply [0], per dependent
 * multiply+add pair [1], per dependent L2 round trip (L1-bypassing pointer chase) [2], per dependent LDS read [3] and
 * per fp64 IEEE division in a dependent chain [4], each measured on one wave */
int ttx_k_latency_probe(int32_t device, double out[5]);

/* RCCL loop-back self-test on one device (pools without a second GPU): a one-rank communicator, a grouped ncclSend / ncclRecv of
 * a msg_bytes message to itself, the MAX all-reduce of 4 doubles and a SUM all-reduce of nsum doubles, all on a non-blocking
 * stream as in the multi-GPU data path (ttx_comm_init, lib/dmrgg.f90:763-958 replaced); TTX_OK when every byte came back */
int ttx_k_rccl_selftest(int32_t device, int64_t msg_bytes, int32_t nsum);

/* placement probe: the XCD (XCC_ID hardware register) on which each of `nblocks` workgroups of a plain 1-D launch
 * ran; the cluster sweep kernel relies on workgroups being dealt round-robin to the 8 XCDs */
int ttx_k_xcc_map(int32_t device, int32_t nblocks, int32_t *out);

#ifdef __cplusplus
}
#endif
#endif
