// ttx_engine.hip -- host orchestration + C-ABI (include/ttx.h) of the MI355X TT-cross engine.
//
// One engine = one dtt_dmrgg problem (reference lib/dmrgg.f90:11-1050).  The sweep is a stream-ordered
// chain of kernels with NO host round trip inside a sweep: the data-dependent control flow of the rook
// loop (lib/dmrgg.f90:516-582) lives in device-side step states that each kernel resolves from the
// previous kernel's partial arg-max records.  The host synchronises once per sweep to read the
// reference's per-sweep report line and to apply the stop rule (lib/dmrgg.f90:1010-1019).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>    // hipExtLaunchKernel: a launch whose completion signal is an event (end_side)

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <atomic>
#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: the library is dlopen()ed by ttx_comm_init

#include "../../include/ttx.h"
#include "../../include/ttx_device_fun.h"   // the slot ABI of loadable device integrands (TTX_FUN_DEVICE)
#include "ttx_err.h"
#include "ttx_lds.h"
#include "ttx_qr_plan.h"
#include "ttx_create_plan.h"
#include "ttx_loop_plan.h"
#include "ttx_shm.h"
#include "ttx_host_pool.h"
#include "ttx_files.h"
#include "ttx_init.h"
#include "ttx_kernels.h"
#include "ttx_wavestep.h"
#include "ttx_de.h"
#include "ttx_mvn.h"
#include "ttx_quadfin.h"
#include "ttx_exchange.h"
#include "ttx_sweep_end.h"
#include "ttx_ttops.h"
#include "ttx_fused.h"
#include "ttx_cluster.h"
#include "ttx_coscoeff.h"
#include "ttx_eval.h"
#include "ttx_contract.h"
#include "ttx_modeapply.h"
#include "ttx_basis.h"
#include "ttx_basis_grad.h"
#include "ttx_basis_core_grad.h"
#include "ttx_sq_norm.h"
#include "ttx_basis_jvp.h"
#include "ttx_basis_enrich.h"
#include "ttx_fit_plan.h"
#include "ttx_algebra.h"
#include "ttx_roundsum.h"
#include "ttx_sample.h"
#include "ttx_sample_real.h"
#include "ttx_topk.h"
#include "ttx_sample_sq.h"
#include "ttx_sample_sq_real.h"
#include "ttx_trainfun.h"
#include "ttx_pullback.h"

// the instantiation of the cluster kernel an engine runs (ttx_engine::cluster_var)
typedef void (*cluster_kernel_t)(DevProb, int, int, int, int, int, int);
static cluster_kernel_t cluster_kernel(int var)
{
    return var == 2 ? k_sweep_cluster<true, false> : var == 1 ? k_sweep_cluster<false, true> : k_sweep_cluster<false, false>;
}


// switches from the environment: an integer (or the default where the variable is unset), "set to 0"
static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
static bool env_off(const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; }

// raise a kernel's dynamic-LDS ceiling on `device` (the current one) to `need` bytes, unless an earlier request there was as large
static int ensure_lds(int device, const void *fn, size_t need)
{
    return ttx_lds_raise(device, fn, need, [](const void *fn, size_t need) -> int {
        HIPCHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        return TTX_OK;
    });
}

extern "C" const char *ttx_last_error(void) { return g_err.c_str(); }
extern "C" int ttx_version(void) { return 3; }      // 2: loadable device integrands; 3: ttx_ijk_batch, ttx_ijk_batch_dev, ttx_value_batch (ttx_contract, ttx_marginals: added without a new number)


// RCCL entry points, resolved at run time (single-GPU users never load librccl)
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi g_rccl;
static int rccl_load()
{
    if (g_rccl.lib) return TTX_OK;
    void *L = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!L) L = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!L) return fail(TTX_EHIP, "cannot load librccl.so: %s", dlerror());
#define SYM_(f, name) *(void **)(&g_rccl.f) = dlsym(L, name); if (!g_rccl.f) return fail(TTX_EHIP, "librccl.so lacks %s", name);
    SYM_(GetUniqueId, "ncclGetUniqueId") SYM_(CommInitRank, "ncclCommInitRank") SYM_(CommDestroy, "ncclCommDestroy")
    SYM_(Send, "ncclSend") SYM_(Recv, "ncclRecv") SYM_(AllReduce, "ncclAllReduce") SYM_(GroupStart, "ncclGroupStart")
    SYM_(GroupEnd, "ncclGroupEnd") SYM_(GetErrorString, "ncclGetErrorString")
#undef SYM_
    g_rccl.lib = L;
    return TTX_OK;
}
#define NCCLCHECK(x) do { ncclResult_t e_ = (x); if (e_ != ncclSuccess) return fail(TTX_EHIP, "%s failed: %s", #x, g_rccl.GetErrorString(e_)); } while (0)

// Operations on the resident train (ttx_eval.h, ttx_contract.h, ttx_algebra.h, ttx_sample.h, ttx_modeapply.h) share one table of device work space
// per engine, grown on demand (buf_reserve), freed in ttx_destroy.  A slot belongs to one role; two roles share a slot only where no
// single call uses both, because a second buf_reserve of a slot may move what the first one handed out.  ttx_sample_real is the widest
// call, then ttx_sample: SC_TRAIN, SC_META, SC_W, SC_M, SC_VEC, SC_H, SC_ROW, SC_CNT and the staging slots (with SC_SRX) are all live in it.  ttx_topk keeps SC_TRAIN,
// SC_META (its per-mode tables) and all seven SC_K* slots live from its first launch to its last copy, reserves each of them once,
// before the first launch, and touches no other slot: what ttx_sample or ttx_marginals left in theirs stays as it was.  ttx_sample_sq keeps
// SC_META (weights, fixed), its four SC_Q* slots, SC_CNT and the staging slots of ttx_sample live, each reserved once before its first use.
enum {
    SC_TRAIN,                           // the EvTrain block (ev_train): evaluation and sampling
    SC_META,                            // a call's tables (OpMeta): contraction, marginals, sampling; the AlgBlk table of the algebra
    SC_IND, SC_OUT, SC_X,               // staging of the host entries: index rows, values (also the marginals), coordinates or uniforms
    SC_FLAG, SC_LQ,                     // ttx_value_batch's flags, ttx_sample's logq
    SC_XA, SC_XB, SC_SORT,              // MFMA evaluation: the two state buffers, the bucket sort
    SC_W, SC_M, SC_P, SC_SCR, SC_VEC,   // contraction: weights, M matrices, run products, their overflow, the l and s vectors
    SC_H, SC_ROW, SC_CNT,               // sampling: head tables, global rows of long modes, the failure counter
    SC_SRX,                             // ttx_sample_real: staging of the drawn coordinates (its uniforms go to SC_X, cell rows to SC_IND, nodes to SC_META)
    SC_TFUN, SC_TVAL,                   // TTX_FUN_TRAINS: the operands' blocks (core pointers, ranks) of a run, the values for a loaded combiner
    SC_PB, SC_PBREF, SC_PBVAL,          // TTX_FUN_PULLBACK: the layers' blocks of a call (plan rows, offsets, core pointers, ranks), the reference rows of the set, the rows x, logq, val for the combiner
    SC_MAT,                             // ttx_mode_apply: the matrices of the applied modes (its tables go to SC_META)
    SC_KP, SC_KW, SC_KS, SC_KX,         // ttx_topk: the Gram matrices P_0 .. P_(d-1), the W of a Gram step, a mode's score sheet (keys), the two state buffers
    SC_KREC, SC_KSEL, SC_KOUT,          // ttx_topk: the kept positions of every mode, the selection's state (words, chunk counts, histogram), the rows before and after the ordering
    SC_RSO, SC_RSW, SC_RSYA, SC_RSYB,   // ttx_lincomb_round: the sketch train Omega, the stacked W of all bonds, the two Y buffers
    SC_RSM, SC_RSTAB,                   // ttx_lincomb_round: M = Q^T Y (first the coefficients), the descriptor tables (RsBlk) and Omega's offsets
    SC_QH, SC_QF, SC_QS, SC_QX,         // ttx_sample_sq: the tables H_k, the factors F_k (then the exponent and the d defensive terms), a mode's sheet (two for ttx_sample_sq_real), the states (two buffers, logq, flags)
    SC_BTAB,                            // ttx_basis_batch: the table of one mode for one chunk, chunk x max n (its states go to SC_XA / SC_XB, its nodes to SC_META)
    SC_GST,                             // ttx_basis_grad_batch: the state store, the rows D_i of all modes of a chunk (its tables go to SC_BTAB, its states to SC_XA / SC_XB)
    SC_CGG, SC_CGP,                     // ttx_basis_core_grad_batch: the packed gradient of a host caller (also ttx_cores_axpy's), the partial blocks of a core's segments (its states X_i go to SC_GST, L to SC_XA / SC_XB)
    SC_JVV, SC_VDP, SC_VIN,             // ttx_basis_jvp_batch: the packed direction of a host caller; ttx_cores_dot: the segment sums, the two buffers of a host caller
    SC_FITV, SC_FITP,                   // ttx_basis_fit_batch: the core-space work vectors and the snapshot; the point vectors, then the uploaded inputs of a host caller
    SC_SQNW, SC_SQNP, SC_SQNY, SC_SQNPT, // ttx_sq_lognorm_grad: the W store; the PR store, the two PL and the exponents; Y of a right step and the per-index partial matrices of a step; ttx_sq_nll_batch: the point vectors, then the uploaded inputs of a host caller
    SC_SQMP, SC_SQMC, SC_SQMW,          // ttx_sq_moments: the PR and PL stores, the exponents, RA, the products and the band; the carried matrices (two sets) and their exponents; the W and partial matrices of a batched launch (its unbatched steps use SC_SQNY)
    SC_ENY, SC_ENS,                     // ttx_basis_enrich_batch: the packed sketches Y_i (then the new directions Q_i); the segment sums and maxima of every bond, then the descriptor tables
    SC_NBUF
};
struct EvBuf { void *p = nullptr; size_t bytes = 0; };
// an event pair around a launch, created on first use
struct OpTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    int start(hipStream_t s) { for (auto &e : ev) if (!e) HIPCHECK(hipEventCreate(&e)); HIPCHECK(hipEventRecord(ev[0], s)); return TTX_OK; }
    int stop(hipStream_t s) { HIPCHECK(hipEventRecord(ev[1], s)); return TTX_OK; }
    int ms(double *out) { float t = 0.f; HIPCHECK(hipEventElapsedTime(&t, ev[0], ev[1])); *out = t; return TTX_OK; }   // after a synchronise
};
enum { TM_MODESUM, TM_ALG, TM_HEAD, TM_DRAW, TM_APPLY,             // k_ct_modesum, the algebra launch, k_sm_head, the k_sm_draw / k_sr_draw of a chunk, k_ma_apply
       TM_GRAM, TM_SCORE, TM_SELECT,                               // ttx_topk: the Gram chain, a mode's scoring launch, a mode's selection and advance
       TM_RS_SKETCH, TM_N };                                       // ttx_lincomb_round: the right-to-left pass (the GEMMs, QRs and advances alternate d - 1 times: OpMarks)
// Events between the phases of a call whose phases alternate many times inside one enqueued stretch, which one OpTimer pair per phase
// cannot time: mark(phase) closes the stretch since the previous mark; after a synchronise, sum() adds every stretch to ms[its phase]
// (DISCARD: to nothing) and empties the chain.  The events are the engine's (ttx_engine::op_ev): created once, reused by every call.
struct OpMarks {
    enum { DISCARD = -1 };
    std::vector<hipEvent_t> &pool;
    std::vector<int> phase;
    explicit OpMarks(std::vector<hipEvent_t> &p) : pool(p) {}
    int mark(hipStream_t s, int ph)
    {
        if (phase.size() == pool.size()) { hipEvent_t e; HIPCHECK(hipEventCreate(&e)); pool.push_back(e); }
        HIPCHECK(hipEventRecord(pool[phase.size()], s));
        phase.push_back(ph);
        return TTX_OK;
    }
    int sum(double *ms)
    {
        for (size_t x = 1; x < phase.size(); x++) {
            if (phase[x] == DISCARD) continue;
            float t = 0.f;
            HIPCHECK(hipEventElapsedTime(&t, pool[x - 1], pool[x]));
            ms[phase[x]] += t;
        }
        phase.clear();
        return TTX_OK;
    }
};

// the figures of an operation's last call, one record each, handed out by the operation's _last entry
// samplers: ttx_sample and ttx_sample_real fill head, bytes and draw, the squared samplers head, rows, pick, flops and mode
enum { SMP_GRID, SMP_REAL, SMP_SQ, SMP_SQ_REAL, SMP_ROS_SQ_REAL, SMP_N };
struct SampleLast { double ms_head = 0.0, bytes = 0.0, ms_draw = 0.0, ms_rows = 0.0, ms_pick = 0.0, flops = 0.0; int64_t failed = 0; int mode = -1; };
struct CtLast { double ms = 0.0, bytes = 0.0; };                               // the mode-sum kernel of ttx_contract / ttx_marginals
struct AlgLast { double ms = 0.0, rd = 0.0, wr = 0.0; };                       // ttx_lincomb / ttx_hadamard with this engine first
struct MaLast { double ms = 0.0, rd = 0.0, wr = 0.0, flops = 0.0; int mode = -1; };    // the apply launch of ttx_mode_apply
struct TkLast { double ms_gram = 0.0, ms_score = 0.0, ms_select = 0.0, flops = 0.0; int mode = -1; };
struct RsLast {                                                                 // ttx_lincomb_round with this engine first
    double ms[4] = {0.0, 0.0, 0.0, 0.0}, flops = 0.0;                           // sketch, gemm, qr, advance
    std::vector<int32_t> l;                                                     // its sketch ranks l(0 .. d)
    int mode = -1;
};
struct BsLast { double ms[2] = {0.0, 0.0}, flops = 0.0; int mode = -1; };      // ttx_basis_batch / ttx_basis_tab: table launches, chain launches
struct BgLast { double ms[3] = {0.0, 0.0, 0.0}, flops = 0.0; int mode = -1; int64_t chunk = 0; };     // ttx_basis_grad_batch / ttx_basis_grad_tab: table, backward, forward launches

struct CgLast { double ms[4] = {0.0, 0.0, 0.0, 0.0}, flops = 0.0; int mode = -1; int64_t chunk = 0; };     // ttx_basis_core_grad_batch / _tab: table, backward, forward, accumulation launches

struct EnLast { double ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, flops = 0.0; int mode = -1; int64_t chunk = 0; };     // ttx_basis_enrich_batch / _tab: table, backward, sketch (forward advance, z, Y, statistics), QR, assembly launches

struct JvLast { double ms[2] = {0.0, 0.0}, flops = 0.0; int mode = -1; };      // ttx_basis_jvp_batch / ttx_basis_jvp_tab: table launches, chain launches
struct FitLast { double ms[4] = {0.0, 0.0, 0.0, 0.0}; int64_t n_jvp = 0, n_cg = 0; int mode = -1; };      // ttx_basis_fit_batch / _tab: JVP, core-gradient, value, vector launches

struct SqnLast { double ms[3] = {0.0, 0.0, 0.0}, flops = 0.0; int mode = -1; };               // ttx_sq_lognorm_grad: right chain, left chain, assembly
struct SqmLast { double ms[4] = {0.0, 0.0, 0.0, 0.0}, flops = 0.0; int64_t steps = 0; int mode = -1; };    // ttx_sq_moments: chains, band, carry, close

struct DevFun;                          // a loaded device integrand (TTX_FUN_DEVICE), defined with slot_eval
struct TrainFun;                        // the operands and the combiner of TTX_FUN_TRAINS, defined with slot_eval
struct PullFun;                         // the layers, the reference grid and the combiner of TTX_FUN_PULLBACK, defined with slot_eval
struct ttx_engine {
    ttx_config cfg;
    std::vector<int32_t> n1;            // 1-based n, size d+2
    std::vector<double> par, aux, quadw;
    std::vector<int32_t> own;           // own[0..nproc]
    int d = 0, RM = 0, NM = 0, G = 0, NC = 0, nbmax = 0, H = 0, mode = 0;
    int g0 = 0;                         // first global group held by this process
    int W = 1, wrank = 0;               // processes (GPUs) of the job, my index
    DevProb P{};
    hipStream_t stream = nullptr;
    std::vector<void *> allocs;
    size_t SB = 0, QB = 0;              // doubles in the summary / quadrature gather buffers
    double *h_sum = nullptr;            // pinned [SB]
    char *h_msg = nullptr;              // pinned 4*MSZ (host-callback transport staging)
    double *h_tmp = nullptr;            // pinned max(QB, SB)
    char *recvL = nullptr, *recvR = nullptr;   // device receive buffers for remote neighbours
    // transports between GPUs: RCCL (device buffers, stream-ordered) or host callbacks (staged through pinned memory)
    ncclComm_t comm = nullptr;
    ttx_transport cb{};
    bool have_cb = false;
    int cb_error = 0;                   // set by a failed host-function transfer (checked at the next host synchronisation)
    // staging of host-transport all-reduces: a ring of pinned slots, one per reduction in flight
    struct RedJob { ttx_engine *h; double *buf; size_t count; int op; };
    static const int NRED = 16;
    RedJob red[NRED];
    double *red_mem = nullptr; size_t red_cap = 0; int red_next = 0;
    RedJob *red_slot(size_t count, int op)
    {
        if (!red_mem || count > red_cap) return nullptr;
        RedJob *j = &red[red_next];
        j->h = this; j->buf = red_mem + (size_t)red_next * red_cap; j->count = count; j->op = op;
        red_next = (red_next + 1) % NRED;
        return j;
    }
    ShmTransport *shm = nullptr;        // built-in node-local transport (ttx_comm_init_shm)
    std::vector<ttx_sweep_rec> recs;
    std::vector<int32_t> tapes;         // [nsweeps-1][d+1][4]
    std::vector<int32_t> rfinal;
    std::vector<std::vector<uint8_t>> updhist;
    int64_t neval = 0;
    double seconds = 0.0;
    bool ran = false;
    // profiling
    bool profile = false;
    struct Ev { int kind, n; hipEvent_t a, b; };
    std::vector<Ev> evs;
    std::vector<hipEvent_t> evpool;
    int64_t k_launches[TTX_K_NKINDS] = {0};
    double k_ms[TTX_K_NKINDS] = {0}, k_bytes[TTX_K_NKINDS] = {0};
    // tt_lib utilities: compact work buffers, allocated on first use
    double *Wa = nullptr, *Wb = nullptr, *Wc = nullptr, *Wd = nullptr, *Sm = nullptr, *bak = nullptr;
    int *Si = nullptr;
    // what creation decided (ttx_create_plan.h): derived sizes, kernel variants, LDS sizes.  Fixed for the life of the engine; what a
    // fallback of ttx_run takes out of use is recorded in `retired`, and the readers ask through the three functions below
    CreatePlan sel;
    struct Retired { bool cluster = false, de_team = false, de_v5 = false; } retired;   // with the cluster path goes Ising C's P.arith (ttx_run)
    int cluster_nb() const { return retired.cluster ? 0 : sel.cluster; }   // workgroups per bond group of the cluster sweep kernel; 0: not used
    bool de_team() const { return sel.de_team && !retired.de_team; }       // Ising D/E half-steps by wave teams (k_halfstep_det)
    bool de_v5() const { return sel.de_v5 && !retired.de_v5; }             // ... by a relay of four waves (k_halfstep_de5)
    int arith() const { return P.arith; }                                  // sel.arith, less Ising C's closed form once the cluster path is retired
    int cluster_fallbacks = 0;          // runs replayed on the chain path after a cluster abort
    int det_fallbacks = 0, de5_fallbacks = 0;   // ... without teams, without the relay
    bool cluster_aborted = false;
    // ev_tail as the tail launch's own completion signal (sel.tail_event_kernel): once the extended launch is refused, the engine records
    // the event behind a plain launch for the rest of its life
    bool tail_event_retired = false; int tail_event_fallbacks = 0;
    double *h_svd = nullptr; double svd_seq = 0.0;   // pinned: [seq, rank, sweeps, sv...] of the core dtt_svd works on (k_svd_report)
    hipStream_t qstream = nullptr;      // forked per-sweep quadrature (single-process runs)
    hipEvent_t ev_sum[2] = {nullptr, nullptr}, ev_val[2] = {nullptr, nullptr}, ev_tail[2] = {nullptr, nullptr}, ev_qb[2] = {nullptr, nullptr}, ev_fin[2] = {nullptr, nullptr};
    double *h_sum_base = nullptr;       // pinned [2][SB]: summaries of the two sweeps in flight
    double *h_val = nullptr;            // pinned [2]: per-sweep quadrature values
    int *h_abort = nullptr;             // pinned, device-visible: the cluster kernel's barrier-timeout flag
    // user integrand evaluated on the host (TTX_FUN_HOST): see DevProb::hostpass
    ttx_host_fun hfun = nullptr;
    const double *hfun_par = nullptr;   // the caller's par(*), passed through untouched
    // user integrand evaluated on the device by a code object the caller loaded (TTX_FUN_DEVICE): shared with replicas
    std::shared_ptr<DevFun> dfun;
    // integrand g(x_1(i), .., x_m(i)) of resident trains (TTX_FUN_TRAINS): operand handles and combiner, shared with replicas; the
    // operands' device blocks as this engine's run sees them (tf_prepare), the figures of ttx_trainfun_last
    std::shared_ptr<TrainFun> tfun;
    TfOps tf_ops{};
    std::vector<char> tf_host;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tf_evs;
    bool tf_figures = false;            // the call in flight records the figures of ttx_trainfun_last (ttx_run, ttx_eval_device; not ttx_accchk)
    int64_t tf_launches = 0, tf_elements = 0;
    double tf_ms = 0.0;
    // integrand of a point pulled back through resident transports (TTX_FUN_PULLBACK): layer handles, node rows, reference grid and
    // combiner, shared with replicas; the layers' device blocks and the launch shape as this engine's call sees them (pb_prepare).  The
    // figures of ttx_pullback_last are TTX_FUN_TRAINS's (tf_*; an engine is one or the other) and the failed count
    std::shared_ptr<PullFun> pfun;
    const PullFun *pb_ref_of = nullptr; // whose reference rows SC_PBREF holds
    PbOps pb_ops{};
    PbPlan pb_pl;
    std::vector<char> pb_host;
    int64_t pb_failed = 0;
    int64_t host_calls = 0;
    int64_t n_resid = 0;                // rook half-steps of the last run that took a residual (all groups)
    // operations on the resident train: work space (SC_*), the host images behind SC_TRAIN and SC_META, timers (TM_*), last figures
    EvBuf scratch[SC_NBUF];
    std::vector<char> train_host, meta_host;
    OpTimer timer[TM_N];
    int ncu = 0;                        // compute units of the device, asked for once (dev_ncu)
    int ev_last_mode = -1;              // TTX_EVAL_* the last batch ran with
    SampleLast smp[SMP_N];                              // the last call of each of the four samplers and of ttx_rosenblatt_sq_real, each its own
    CtLast ct;
    AlgLast alg;
    MaLast ma;
    TkLast tk;
    RsLast rs;
    BsLast bs;
    BgLast bg;
    CgLast cg;
    EnLast en;
    JvLast jv;
    FitLast fit;
    SqnLast sqn;
    SqmLast sqm;
    std::vector<hipEvent_t> op_ev;                      // OpMarks' events: ttx_lincomb_round, the squared samplers, the basis evaluations
};

// the process-wide pool of the host integrand (ttx_host_pool.h): engines driven from different host threads take turns on it
static HostPool &host_pool()
{
    static HostPool p(host_pool_threads(getenv("TTX_HOST_THREADS"), getenv("OMP_NUM_THREADS"), std::thread::hardware_concurrency()));
    return p;
}

// after the index pass of a kernel: wait for it, call the user's function for every requested slot, clear the requests
static int host_eval(ttx_engine *h)
{
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    DevProb &P = h->P;
    const size_t nslot = (size_t)h->G * h->sel.HS;
    std::vector<uint32_t> todo;
    for (size_t s = 0; s < nslot; s++) if (P.hreq[s]) { todo.push_back((uint32_t)s); P.hreq[s] = 0; }
    const int32_t d = h->d;
    const int32_t *nn = h->n1.data() + 1;
    host_pool().run(todo.size(), [&](size_t i) {
        int32_t ind[2048];
        const short *row = P.hidx + (size_t)todo[i] * d;
        for (int k = 0; k < d; k++) ind[k] = row[k];
        P.hval[todo[i]] = h->hfun(&d, ind, nn, h->hfun_par);
    });
    h->host_calls += (int64_t)todo.size();
    return TTX_OK;
}

// ---- TTX_FUN_DEVICE: the integrand is a code object the caller compiled against include/ttx_device_fun.h ---------------------
// The module, its two kernels and the device copy of the caller's par; an engine and its replicas (ttx_replicate) share one.
struct DevFun {
    int device = 0;
    hipModule_t mod = nullptr;
    hipFunction_t slots = nullptr, list = nullptr;
    ttx_devfun_info info{};
    double *par = nullptr;
    std::string name;
    std::vector<unsigned char> image;           // the loader's private copy of the code object: lives as long as the module
    ~DevFun()
    {
        (void)hipSetDevice(device);
        if (par) (void)hipFree(par);                // hipFree waits for the device: no kernel of the module is in flight after it
        else (void)hipDeviceSynchronize();
        if (mod) (void)hipModuleUnload(mod);
    }
};
#define DEVFUN_LAUNCHCHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(TTX_EHIP, "%s failed: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
// the loaded slot kernel over all slots of this process, on the stream behind pass 1 (no synchronisation).  Launch shape (the
// header's contract): workgroups of info.block threads; lane form one lane per slot, wave
// form one wave per slot; both capped (the kernels stride), with info.lds_per_wave bytes of LDS per wave
static int devfun_slots(ttx_engine *h)
{
    DevFun &f = *h->dfun;
    DevProb &P = h->P;
    int d = P.d;
    long long nslot = (long long)h->G * h->sel.HS;
    const int *n = P.n + 1;
    const double *par = f.par;
    const short *hidx = P.hidx; unsigned char *hreq = P.hreq; double *hval = P.hval;
    const int waves = f.info.block / 64;
    const long long want = f.info.kind == TTX_DEVFUN_KIND_WAVE ? (nslot + waves - 1) / waves : (nslot + f.info.block - 1) / f.info.block;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(want, 4096));
    void *args[] = {&d, &n, &par, &nslot, &hidx, &hreq, &hval};
    DEVFUN_LAUNCHCHECK(hipModuleLaunchKernel(f.slots, grid, 1, 1, (unsigned)f.info.block, 1, 1, (unsigned)(f.info.lds_per_wave * waves), h->stream, args, nullptr));
    return TTX_OK;
}

// ---- TTX_FUN_TRAINS: fun(i) = g(x_1(i), .., x_m(i)) for resident trains x_t (ttx_trainfun.h) ------------------------------------
// The operands are recorded as handles; their device blocks are rebuilt by tf_prepare at the start of every call that evaluates.
struct TrainFun {
    std::vector<ttx_engine *> x;
    int op = 0;
    std::shared_ptr<DevFun> comb;           // TTX_TOP_DEVICE: the loaded combiner (ttx_devcomb_* symbols)
};
static int tf_grid(ttx_engine *h, long long items);
static int tf_prepare(ttx_engine *h, const char *who, bool figures);
static int tf_finish(ttx_engine *h);
static int tf_eval_list(ttx_engine *h, int64_t npts, const int32_t *ind, double *out);
// ---- TTX_FUN_PULLBACK: fun(i) = h(x, logq, val) at the grid point of i pulled back through resident transports (ttx_pullback.h) -----
// Layers are recorded as handles with copies of their node rows; their heads and device blocks are rebuilt by pb_prepare at the start
// of every call that evaluates.
struct PullFun {
    struct Layer { ttx_engine *x; std::vector<std::vector<double>> nodes; double gamma; };
    std::vector<Layer> layer;
    std::vector<double> ref;                // the reference rows, mode k at roff[k]
    std::vector<size_t> roff;
    std::shared_ptr<DevFun> comb;           // null: the layers only (ttx_pullback_points)
};
static int pb_prepare(ttx_engine *h, const char *who, bool figures, bool need_comb);
static int pb_slots(ttx_engine *h);
static int pb_finish(ttx_engine *h);
static int pb_eval_list(ttx_engine *h, int64_t npts, const int32_t *ind, double *out);
// with ttx_set_profile on, an event pair around the launches of one slot evaluation (collected by tf_finish)
struct TfScope {
    ttx_engine *h; hipEvent_t a = nullptr, b = nullptr;
    bool on;
    explicit TfScope(ttx_engine *h_) : h(h_), on(h_->profile && h_->tf_figures) { if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, h->stream); } }
    ~TfScope() { if (on) { (void)hipEventRecord(b, h->stream); h->tf_evs.push_back({a, b}); } }
};
// k_tf_slots over all slots of this process behind pass 1, and for a loaded combiner its slot kernel behind that: no synchronisation
static int tf_slots(ttx_engine *h)
{
    const TrainFun &f = *h->tfun;
    DevProb &P = h->P;
    long long nslot = (long long)h->G * h->sel.HS;
    const TfOps &O = h->tf_ops;
    const size_t lds = sizeof(double) * TTX_TF_WAVES * tf_lds_doubles(O.ldx, O.d);
    const dim3 grid(tf_grid(h, nslot)), block(64 * TTX_TF_WAVES);
    const short *hidx = P.hidx; unsigned char *hreq = P.hreq; double *hval = P.hval;
    double *tval = (double *)h->scratch[SC_TVAL].p;
    unsigned long long *cnt = (unsigned long long *)h->scratch[SC_CNT].p;
    if (h->tf_figures) h->tf_launches++;
    TfScope timed(h);
    switch (f.op) {
        case TTX_TOP_PRODUCT: hipLaunchKernelGGL(k_tf_slots<TF_PRODUCT>, grid, block, lds, h->stream, O, nslot, hidx, hreq, hval, tval, cnt); break;
        case TTX_TOP_RATIO: hipLaunchKernelGGL(k_tf_slots<TF_RATIO>, grid, block, lds, h->stream, O, nslot, hidx, hreq, hval, tval, cnt); break;
        case TTX_TOP_SQRTABS: hipLaunchKernelGGL(k_tf_slots<TF_SQRTABS>, grid, block, lds, h->stream, O, nslot, hidx, hreq, hval, tval, cnt); break;
        default: {
            hipLaunchKernelGGL(k_tf_slots<TF_DEVICE>, grid, block, lds, h->stream, O, nslot, hidx, hreq, hval, tval, cnt);
            DevFun &c = *f.comb;
            int m = O.m, d = O.d;
            const int *n = P.n + 1;
            const double *par = c.par, *tv = tval;
            const unsigned cg = (unsigned)std::max<long long>(1, std::min<long long>((nslot + c.info.block - 1) / c.info.block, 4096));
            void *args[] = {&m, &d, &n, &par, &nslot, &hidx, &hreq, &tv, &hval};
            DEVFUN_LAUNCHCHECK(hipModuleLaunchKernel(c.slots, cg, 1, 1, (unsigned)c.info.block, 1, 1, 0, h->stream, args, nullptr));
        }
    }
    return TTX_OK;
}

// between the two passes of an evaluating kernel: the host's `fun` (host_eval), or for TTX_FUN_COSCOEFF the device evaluator over
// the requested slots, enqueued on the stream behind pass 1 (no synchronisation)
static int slot_eval(ttx_engine *h)
{
    DevProb &P = h->P;
    if (!P.slot_dev) return host_eval(h);
    if (h->cfg.fun_id == TTX_FUN_DEVICE) return devfun_slots(h);
    if (h->cfg.fun_id == TTX_FUN_TRAINS) return tf_slots(h);
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) return pb_slots(h);
    const long long nslot = (long long)h->G * h->sel.HS;
    const unsigned grid = (unsigned)std::min<long long>((nslot + TTX_CC_WAVES - 1) / TTX_CC_WAVES, 1024);
    hipLaunchKernelGGL(k_coscoeff_slots, dim3(grid), dim3(64 * TTX_CC_WAVES), sizeof(double) * TTX_CC_WAVES * TTX_CC_LDS(P.d), h->stream,
                       P.d, P.aux, nslot, (const short *)P.hidx, P.hreq, P.hval);
    return TTX_OK;
}


template <class T>
static int dev_alloc(ttx_engine *h, T **p, size_t count)
{
    void *q = nullptr;
    HIPCHECK(hipMalloc(&q, count * sizeof(T) + 64));
    HIPCHECK(hipMemset(q, 0, count * sizeof(T) + 64));
    // the fill runs on the null stream, which is NOT ordered against the engine's non-blocking stream: finish it
    // here, or a buffer allocated on first use could be zeroed after the first kernel has written it
    HIPCHECK(hipDeviceSynchronize());
    h->allocs.push_back(q);
    *p = (T *)q;
    return TTX_OK;
}

// the restated figures of ttx_create_plan.h against the kernel headers'
static_assert(TTX_EN_STORAGE == TTX_MAXPART * TTX_BLK, "ttx_op_plan.h restates TTX_MAXPART * TTX_BLK");
static_assert(TTX_PLAN_FB == FB && TTX_PLAN_FNR == TTX_FNR && TTX_PLAN_MVN_MAXQ == MVN_MAXQ, "ttx_create_plan.h restates FB, TTX_FNR, MVN_MAXQ");

static int ensure_lds(const ttx_engine *h, const void *fn, size_t need) { return ensure_lds(h->cfg.device, fn, need); }
static int ensure_lds_cluster(ttx_engine *h) { return ensure_lds(h, reinterpret_cast<const void *>(cluster_kernel(h->sel.cluster_var)), h->sel.lds_cluster); }

static void destroy_keep_error(ttx_engine *e) { const std::string msg = g_err; ttx_destroy(e); g_err = msg; }

// the environment switches of engine creation: the one place of the create path that calls getenv
static CreateEnv create_env() { return create_env_from([](const char *name) -> const char * { return getenv(name); }); }

// ---- what creation allocates, by purpose; every size comes from the plan (h->sel) ------------------------------------------------
#define A_(call) do { if (int rc_ = (call)) return rc_; } while (0)
template <class T>
static int dev_upload(ttx_engine *h, T **p, const T *src, size_t count)
{
    A_(dev_alloc(h, p, count));
    HIPCHECK(hipMemcpy(*p, src, sizeof(T) * count, hipMemcpyHostToDevice));
    return TTX_OK;
}
// the problem as the caller gave it: mode sizes, par, aux, quadrature weights; DevProb's scalars, filled from the plan here
static int create_problem(ttx_engine *h)
{
    const CreatePlan &s = h->sel;
    const ttx_config &cfg = h->cfg;
    DevProb &P = h->P;
    const int d = s.d, NM = s.NM;
    P.d = d; P.RM = s.RM; P.NM = NM; P.G = s.G; P.NC = s.NC; P.g0 = s.g0;
    P.fun_id = cfg.fun_id; P.piv = cfg.pivoting; P.npar = cfg.npar; P.nprocs = s.nproc;
    P.ising_id = s.ising_id;
    P.has_quad = cfg.quadw != nullptr;
    P.small_element = 10 * 2.220446049250313e-16; P.small_pivot = 1.e-5;   // lib/dmrgg.f90:70-71
    P.mvn_norm = s.mvn_norm;
    P.SS = s.SS; P.SW = s.SW; P.CS = s.CS;
    P.arith = s.arith; P.FD = s.FD; P.fpersist = s.fpersist;
    P.de_npair = s.de_npair; P.de_unit = s.de_unit; P.de_cut = s.de_cut;
    P.nfb = s.nfb; P.fp_mfma = s.fp_mfma; P.fp_tiles = s.fp_tiles;
    P.XD = s.XD; P.IOFF = s.IOFF; P.MSZ = s.MSZ;
    P.accuracy = cfg.accuracy; P.maxrank = cfg.maxrank;
    P.lot_nb = s.lot_nb; P.lot_max = s.nlotmax; P.bnd_wave = s.bnd_wave;
    h->n1.assign(d + 2, 1);
    for (int k = 1; k <= d; k++) h->n1[k] = cfg.n[k - 1];
    if (cfg.npar > 0) h->par.assign(cfg.par, cfg.par + cfg.npar);
    if (cfg.aux && cfg.naux > 0) h->aux.assign(cfg.aux, cfg.aux + cfg.naux);
    int *dn; double *dpar, *daux = nullptr, *dq = nullptr;
    A_(dev_upload(h, &dn, h->n1.data(), (size_t)d + 2));
    A_(dev_alloc(h, &dpar, cfg.npar + 1));
    if (cfg.npar > 0) HIPCHECK(hipMemcpy(dpar, h->par.data(), sizeof(double) * cfg.npar, hipMemcpyHostToDevice));
    if (!h->aux.empty()) A_(dev_upload(h, &daux, h->aux.data(), h->aux.size()));
    if (cfg.quadw) {
        h->quadw.assign((size_t)(d + 1) * NM, 0.0);
        size_t off = 0;
        for (int k = 1; k <= d; k++) { for (int j = 0; j < h->n1[k]; j++) h->quadw[(size_t)k * NM + j] = cfg.quadw[off + j]; off += h->n1[k]; }
        A_(dev_upload(h, &dq, h->quadw.data(), h->quadw.size()));
    }
    P.n = dn; P.par = dpar; P.aux = daux; P.quadw = dq;
    return TTX_OK;
}
// tables of one integrand: fast arithmetic (ttx_fast.h), Ising D/E pair factors (ttx_de.h), mvn's transposed inverse covariance
static int create_integrand_tables(ttx_engine *h)
{
    const CreatePlan &s = h->sel;
    DevProb &P = h->P;
    const int d = s.d;
    const size_t G = s.G, NC = s.NC, RM = s.RM;
    const bool mvn = h->cfg.fun_id == TTX_FUN_MVN;
    if (s.fast_tables) {
        const size_t slots = s.fpersist ? G * NC : G;
        for (int sd = 0; sd < 2; sd++) {
            A_(dev_alloc(h, &P.fNear[sd], slots * (size_t)s.FD * RM));
            A_(dev_alloc(h, &P.fPiv[sd], slots * (size_t)TTX_FS * RM));
            if (mvn) A_(dev_alloc(h, &P.fDv[sd], slots * (size_t)s.FD * RM));
        }
        if (mvn) {
            std::vector<double> sy((size_t)d * d);
            const double *ic = h->aux.data() + d;
            for (int i = 0; i < d; i++) for (int j = 0; j < d; j++) sy[i + (size_t)d * j] = 0.5 * (ic[i + (size_t)d * j] + ic[j + (size_t)d * i]);
            double *ds;
            A_(dev_upload(h, &ds, sy.data(), sy.size()));
            P.auxS = ds;
        }
    }
    if (s.de_npair) {
        A_(dev_alloc(h, &P.deTL, G * (size_t)s.de_npair * RM)); A_(dev_alloc(h, &P.deTR, G * (size_t)s.de_npair * RM));
        A_(dev_alloc(h, &P.deUL, G * (size_t)(d + 1) * RM));
        if (s.de_cut) { A_(dev_alloc(h, &P.deCL, G * (size_t)(d + 1) * RM)); A_(dev_alloc(h, &P.deCR, G * (size_t)(d + 1) * RM)); }
    }
    if (mvn) {
        std::vector<double> t((size_t)d * d);
        for (int i = 0; i < d; i++) for (int j = 0; j < d; j++) t[j + (size_t)d * i] = h->aux[d + i + (size_t)d * j];
        double *dt;
        A_(dev_upload(h, &dt, t.data(), t.size()));
        P.auxT = dt;
    }
    return TTX_OK;
}
// cores, factors, index tables and per-group state; the searches' records; the lottery's CDF tables and work space
static int create_cores(ttx_engine *h)
{
    const CreatePlan &s = h->sel;
    DevProb &P = h->P;
    const size_t d = s.d, G = s.G, NC = s.NC, RM = s.RM, NM = s.NM;
    A_(dev_alloc(h, &P.arg, G * NC * P.CS)); A_(dev_alloc(h, &P.col, G * NC * P.CS)); A_(dev_alloc(h, &P.row, G * NC * P.CS));
    A_(dev_alloc(h, &P.inv, G * NC * RM * RM)); A_(dev_alloc(h, &P.vip, G * NC * 4 * RM));
    A_(dev_alloc(h, &P.L, G * NC * d * RM)); A_(dev_alloc(h, &P.R, G * NC * d * RM));
    A_(dev_alloc(h, &P.r, G * (d + 2))); A_(dev_alloc(h, &P.rr, G * (d + 2))); A_(dev_alloc(h, &P.upd, G * (d + 2))); A_(dev_alloc(h, &P.tape, G * (d + 2) * 4));
    A_(dev_alloc(h, &P.acol, G * RM * NM)); A_(dev_alloc(h, &P.arow, G * RM * NM));
    A_(dev_alloc(h, &P.Tq, G * NC * RM * RM));
    A_(dev_alloc(h, &P.ind0, d + 2)); A_(dev_alloc(h, &P.gs, G));
    for (size_t g = 0; g < G; g++) {    // the bond range of every local group is fixed for the life of the engine (k_reset leaves it alone)
        GroupState g0s{};
        g0s.first = h->own[h->g0 + g]; g0s.last = h->own[h->g0 + g + 1] - 1; g0s.gglobal = h->g0 + (int)g;
        const hipError_t e = hipMemcpy(P.gs + g, &g0s, offsetof(GroupState, S), hipMemcpyHostToDevice);
        if (e != hipSuccess) return fail(TTX_EHIP, "ttx_create: %s", hipGetErrorString(e));
    }
    if (s.pfull) A_(dev_alloc(h, &P.pfull, G * NM * RM * (size_t)s.nfb));
    if (s.fp_mfma) { A_(dev_alloc(h, &P.sb, G * (RM * NM) * (RM * NM))); A_(dev_alloc(h, &P.pfull2, G * (size_t)s.fp_tiles)); }
    if (s.cdf_kmax >= 0) {
        CdfTables t;
        if (!cdf_tables(s.cdf_kmax, t)) return fail(TTX_EINVAL, "ttx_create: no CDF tables up to K = %d", s.cdf_kmax);     // cdf_table_fits says there are
        ttx_cdfseg *dt; int *dn_;
        A_(dev_upload(h, &dt, t.tab.data(), t.tab.size()));
        A_(dev_upload(h, &dn_, t.ns.data(), t.ns.size()));
        P.cdf_tab = dt; P.cdf_ns = dn_; P.cdf_kmax = s.cdf_kmax;
    }
    LotPart *lp; unsigned *lc;
    A_(dev_alloc(h, &lp, G * s.lot_nb));
    A_(dev_alloc(h, &lc, G));
    P.lotp = lp; P.lot_ctr = lc;
    if (s.lot_cand) { A_(dev_alloc(h, &P.lotc, G * s.nlotmax * 4)); A_(dev_alloc(h, &P.lotf, G * s.nlotmax)); }
    if (s.cluster) {
        unsigned *ctr; ClPart *cp;
        A_(dev_alloc(h, &ctr, G));
        // (behind the records: every group's image of its sorted pivot lists, cl_zimage of ttx_cluster.h)
        A_(dev_alloc(h, &cp, 2 * G * TTX_CLREC + (s.cl_lists ? (G * cl_zimage_ints(s.nbmax, s.RM) * sizeof(int) + sizeof(ClPart) - 1) / sizeof(ClPart) : 0)));
        P.cl_ctr = ctr; P.cl_part = cp;
#ifdef TTX_STAMPS
        if (s.dbg_waves) { long long *dbg; A_(dev_alloc(h, &dbg, (size_t)8 * 64 * 8)); P.dbg = dbg; }
#endif
        HIPCHECK(hipHostMalloc((void **)&h->h_abort, sizeof(int)));
        *h->h_abort = 0;
        P.cl_abort = h->h_abort;
        P.cl_test_abort = s.cl_test_abort;
    }
    return TTX_OK;
}
// neighbour messages and their routing, the reductions of a sweep, the quadrature's gather
static int create_exchange(ttx_engine *h)
{
    const CreatePlan &s = h->sel;
    DevProb &P = h->P;
    const size_t G = s.G, RM = s.RM, d = s.d;
    const int nproc = s.nproc;
    A_(dev_alloc(h, &P.msgR, G * P.MSZ)); A_(dev_alloc(h, &P.msgL, G * P.MSZ));
    A_(dev_alloc(h, &h->recvL, P.MSZ)); A_(dev_alloc(h, &h->recvR, P.MSZ));
    A_(dev_alloc(h, &P.inL, G)); A_(dev_alloc(h, &P.inR, G));
    A_(dev_alloc(h, &P.red, G * 4)); A_(dev_alloc(h, &P.redsend, 4));
    A_(dev_alloc(h, &P.qsend, h->QB)); A_(dev_alloc(h, &P.qwork, ((size_t)nproc + 2) * RM * RM)); A_(dev_alloc(h, &P.sumsend, h->SB));
    P.qscr = nullptr;
    if (s.qscr) A_(dev_alloc(h, &P.qscr, G * 2 * RM * RM));
    if (s.W > 1) { A_(dev_alloc(h, &P.redrecv, 4)); A_(dev_alloc(h, &P.qall, h->QB)); A_(dev_alloc(h, &P.sumrecv, h->SB)); }
    else { P.redrecv = P.redsend; P.qall = P.qsend; P.sumrecv = P.sumsend; }     // one GPU: results alias the inputs
    {   // message routing: neighbour on this GPU -> its send buffer; on another GPU -> the receive buffer
        std::vector<char *> il(G, nullptr), ir(G, nullptr);
        for (size_t g = 0; g < G; g++) {
            if (g > 0) il[g] = P.msgR + (g - 1) * P.MSZ; else if (h->g0 > 0) il[g] = h->recvL;
            if (g + 1 < G) ir[g] = P.msgL + (g + 1) * P.MSZ; else if (h->g0 + (int)G < nproc) ir[g] = h->recvR;
        }
        HIPCHECK(hipMemcpy(P.inL, il.data(), sizeof(char *) * G, hipMemcpyHostToDevice));
        HIPCHECK(hipMemcpy(P.inR, ir.data(), sizeof(char *) * G, hipMemcpyHostToDevice));
    }
    int *ctl, *rq;
    A_(dev_alloc(h, &ctl, (size_t)4));
    A_(dev_alloc(h, &rq, G * (d + 2)));
    P.ctl = ctl; P.rq = rq;
    // records of the end of a sweep by parity (ttx_dev.h: tail_side)
    P.tail_side = 0;
    A_(dev_alloc(h, &P.tailrec, 2 * G)); A_(dev_alloc(h, &P.tail_tape, 2 * G * (d + 2) * 4)); A_(dev_alloc(h, &P.strk, (size_t)2));
    return TTX_OK;
}
// pinned staging of the per-sweep summaries and of the host transports, the quadrature's stream, the events of the pipelined sweep
static int create_staging(ttx_engine *h)
{
    HIPCHECK(hipHostMalloc((void **)&h->h_sum_base, sizeof(double) * 2 * h->SB));
    h->h_sum = h->h_sum_base;
    memset(h->h_sum_base, 0, sizeof(double) * 2 * h->SB);
    HIPCHECK(hipHostMalloc((void **)&h->h_val, sizeof(double) * 2));
    HIPCHECK(hipStreamCreateWithFlags(&h->qstream, hipStreamNonBlocking));
    if (h->sel.lds_qtree) if (int rc = ensure_lds(h, reinterpret_cast<const void *>(k_quad_tree), h->sel.lds_qtree)) return rc;
    for (int x = 0; x < 2; x++) { HIPCHECK(hipEventCreateWithFlags(&h->ev_sum[x], hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&h->ev_val[x], hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&h->ev_tail[x], hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&h->ev_qb[x], hipEventDisableTiming)); HIPCHECK(hipEventCreateWithFlags(&h->ev_fin[x], hipEventDisableTiming)); }
    HIPCHECK(hipHostMalloc((void **)&h->h_msg, 4 * h->P.MSZ));
    HIPCHECK(hipHostMalloc((void **)&h->h_tmp, sizeof(double) * std::max(h->QB, h->SB)));
    if (h->W > 1) {
        h->red_cap = std::max<size_t>(std::max(h->QB, h->SB), 8);
        HIPCHECK(hipHostMalloc((void **)&h->red_mem, sizeof(double) * h->red_cap * ttx_engine::NRED));
    }
    return TTX_OK;
}
// slots of a two-pass integrand: pinned for the host's `fun`; device memory (zero-filled, owned by allocs) where the evaluator
// runs on the stream between the two passes
static int create_slots(ttx_engine *h)
{
    const CreatePlan &s = h->sel;
    DevProb &P = h->P;
    if (s.slots == SLOTS_NONE) return TTX_OK;
    const size_t nslot = (size_t)s.G * s.HS, d = s.d;
    if (s.slots == SLOTS_DEVICE) {
        P.slot_dev = 1;
        A_(dev_alloc(h, &P.hidx, nslot * d)); A_(dev_alloc(h, &P.hval, nslot)); A_(dev_alloc(h, &P.hreq, nslot));
    } else {
        HIPCHECK(hipHostMalloc((void **)&P.hidx, sizeof(short) * nslot * d));
        HIPCHECK(hipHostMalloc((void **)&P.hval, sizeof(double) * nslot));
        HIPCHECK(hipHostMalloc((void **)&P.hreq, nslot));
        memset(P.hreq, 0, nslot); memset(P.hval, 0, sizeof(double) * nslot);
    }
    P.HS = (int)s.HS; P.hostpass = 0;
    return TTX_OK;
}
#undef A_

// nofun: an engine that only holds a tensor train (ttx_from_tt / ttx_read): no integrand, ttx_run refused
static int create_impl(ttx_engine **out, const ttx_config *cfg, bool nofun)
{
    if (!out || !cfg) return fail(TTX_EINVAL, "ttx_create: null argument");
    *out = nullptr;
    if (!cfg->n) return fail(TTX_EINVAL, "ttx_create: mode sizes missing");
    if (cfg->d < 2) return fail(TTX_EINVAL, "dtt_dmrgg: l,m: 1 %d", cfg->d);
    if (cfg->maxrank < 1 || cfg->maxrank > 128) return fail(TTX_EINVAL, "ttx_create: maxrank must be in 1..128 (got %d)", cfg->maxrank);
    if (cfg->pivoting < -1) return fail(TTX_EINVAL, "dtt_dmrgg: unknown pivoting: %d", cfg->pivoting);   // lib/dmrgg.f90:590-592
    if (2 * cfg->pivoting + 2 > TTX_MAXH) return fail(TTX_EINVAL, "dtt_dmrgg: pivoting %d too large", cfg->pivoting);
    if (!(nofun && cfg->fun_id == 0) && (cfg->fun_id < 1 || cfg->fun_id > TTX_FUN_PULLBACK)) return fail(TTX_EINVAL, "ttx_create: unknown fun_id %d", cfg->fun_id);
    if (cfg->npar < 0 || (cfg->npar > 0 && !cfg->par)) return fail(TTX_EINVAL, "ttx_create: par missing");
    if (cfg->fun_id == TTX_FUN_ISING && (cfg->npar < 2 * cfg->n[0] + 1)) return fail(TTX_EINVAL, "ttx_create: the Ising integrand needs par(1:2n+1) (nodes, weights, id)");
    if ((cfg->fun_id == TTX_FUN_STDNORM || cfg->fun_id == TTX_FUN_MVN) && cfg->npar < cfg->n[0]) return fail(TTX_EINVAL, "ttx_create: the integrand needs the nodes par(1:n)");
    // the built-in integrands address par(ind) (and the Ising weights par(n(1) + ind)): no mode may be larger than the first
    // (test_crs_ising.f90:181-183); with the reference this is the caller's business, here it would be a read outside the parameter vector
    // (the COS coefficients do not index par)
    if (cfg->fun_id != TTX_FUN_HOST && cfg->fun_id != TTX_FUN_COSCOEFF && cfg->fun_id != TTX_FUN_DEVICE && cfg->fun_id != TTX_FUN_TRAINS && cfg->fun_id != TTX_FUN_PULLBACK && cfg->fun_id != 0)
        for (int k = 1; k < cfg->d; k++)
            if (cfg->n[k] > cfg->n[0]) return fail(TTX_EINVAL, "ttx_create: mode %d has %d points, more than the first mode (%d): the built-in integrands index par by n(1)", k + 1, cfg->n[k], cfg->n[0]);
    if (cfg->fun_id == TTX_FUN_HOST && cfg->d > 2048) return fail(TTX_EINVAL, "ttx_create: host integrand: at most 2048 dimensions (tt_size)");
    if (cfg->fun_id == TTX_FUN_DEVICE && cfg->d > 2048) return fail(TTX_EINVAL, "ttx_create: device integrand: at most 2048 dimensions (tt_size)");
    if (cfg->fun_id == TTX_FUN_TRAINS && cfg->d > 2048) return fail(TTX_EINVAL, "ttx_create: integrand of trains: at most 2048 dimensions (tt_size)");
    if (cfg->fun_id == TTX_FUN_PULLBACK && cfg->d > 2048) return fail(TTX_EINVAL, "ttx_create: pulled-back integrand: at most 2048 dimensions (tt_size)");
    if (cfg->fun_id == TTX_FUN_COSCOEFF) { if (int rc0 = coscoeff_check("ttx_create", cfg->d, cfg->n, cfg->aux, cfg->naux)) return rc0; }
    const int W = cfg->world_size < 1 ? 1 : cfg->world_size;
    if (cfg->fun_id == TTX_FUN_TRAINS && W > 1) return fail(TTX_EINVAL, "ttx_create: an integrand of trains (TTX_FUN_TRAINS) runs in one process: bond groups (nproc) work, world_size %d does not", W);
    if (cfg->fun_id == TTX_FUN_PULLBACK && W > 1) return fail(TTX_EINVAL, "ttx_create: a pulled-back integrand (TTX_FUN_PULLBACK) runs in one process: bond groups (nproc) work, world_size %d does not", W);
    const int nproc = std::max(cfg->nproc < 1 ? 1 : cfg->nproc, 1);
    if (nproc >= cfg->d) return fail(TTX_EINVAL, "nproc exceeds or equal dimension, cannot proceed");   // lib/dmrgg.f90:114-117
    if (nproc < W) return fail(TTX_EINVAL, "ttx_create: %d bond groups cannot be spread over %d GPUs", nproc, W);
    if (nproc > 256) return fail(TTX_EINVAL, "ttx_create: at most 256 bond groups");
    if (cfg->world_rank < 0 || cfg->world_rank >= W) return fail(TTX_EINVAL, "ttx_create: world_rank out of range");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "ttx_create: no HIP device (the engine has no CPU path)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(TTX_ENODEV, "ttx_create: device %d not present", cfg->device);
    HIPCHECK(hipSetDevice(cfg->device));
    DevCaps caps;
    {
        hipDeviceProp_t prop;
        HIPCHECK(hipGetDeviceProperties(&prop, cfg->device));
        int coop = 0;
        HIPCHECK(hipDeviceGetAttribute(&coop, hipDeviceAttributeCooperativeLaunch, cfg->device));
        caps.ncu = prop.multiProcessorCount; caps.coop = coop != 0;
    }

    // every decision, before anything is allocated: a refusal leaves nothing behind
    ttx_config c = *cfg;
    c.nproc = nproc;
    CreatePlan plan = create_plan(c, nofun, create_env(), caps);
    if (plan.err) return fail(plan.err, "%s", plan.errtext.c_str());
    if (plan.cluster_cand) {
        // residency: what the device can hold of THIS kernel with THIS much dynamic LDS
        const void *fn = reinterpret_cast<const void *>(cluster_kernel(plan.cluster_var));
        if (int rc = ensure_lds(cfg->device, fn, plan.lds_cluster)) return rc;
        int occ = 0;
        HIPCHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, cluster_kernel(plan.cluster_var), CB, plan.lds_cluster));
        create_admit(plan, occ);
    } else create_admit(plan, 0);

    ttx_engine *h = new ttx_engine();
    // every early return below destroys the engine and what it holds so far; the error text is set before and survives
    struct Guard { ttx_engine *h; ~Guard() { if (h) destroy_keep_error(h); } } guard{h};
    h->cfg = c;
    h->sel = std::move(plan);
    const CreatePlan &s = h->sel;
    h->W = s.W; h->wrank = s.wrank; h->d = s.d; h->RM = s.RM; h->NM = s.NM; h->own = s.own;
    h->g0 = s.g0; h->G = s.G; h->nbmax = s.nbmax; h->NC = s.NC; h->mode = s.mode; h->H = s.H;
    h->QB = s.QB; h->SB = s.SB;
    HIPCHECK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    int rc;
    if ((rc = create_problem(h)) || (rc = create_integrand_tables(h)) || (rc = create_cores(h)) || (rc = create_exchange(h)) ||
        (rc = create_staging(h)) || (rc = create_slots(h))) return rc;
    guard.h = nullptr;
    *out = h;
    return TTX_OK;
}
extern "C" int ttx_create(ttx_engine **out, const ttx_config *cfg) { return create_impl(out, cfg, false); }

extern "C" void ttx_destroy(ttx_engine *h)
{
    if (!h) return;
    if (h->dfun) { (void)hipSetDevice(h->cfg.device); if (h->stream) (void)hipStreamSynchronize(h->stream); h->dfun.reset(); }   // the last owner unloads the module
    if (h->tfun) { (void)hipSetDevice(h->cfg.device); if (h->stream) (void)hipStreamSynchronize(h->stream); h->tfun.reset(); }   // ... and a loaded combiner's
    if (h->pfun) { (void)hipSetDevice(h->cfg.device); if (h->stream) (void)hipStreamSynchronize(h->stream); h->pfun.reset(); }
    if (h->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(h->comm);
    for (void *p : h->allocs) (void)hipFree(p);
    for (auto &b : h->scratch) if (b.p) (void)hipFree(b.p);
    for (auto &t : h->timer) for (auto &e : t.ev) if (e) (void)hipEventDestroy(e);
    for (auto &e : h->tf_evs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (h->h_sum_base) (void)hipHostFree(h->h_sum_base);
    if (h->h_val) (void)hipHostFree(h->h_val);
    if (h->h_svd) (void)hipHostFree(h->h_svd);
    if (h->qstream) (void)hipStreamDestroy(h->qstream);
    for (int x = 0; x < 2; x++) { if (h->ev_sum[x]) (void)hipEventDestroy(h->ev_sum[x]); if (h->ev_val[x]) (void)hipEventDestroy(h->ev_val[x]); if (h->ev_tail[x]) (void)hipEventDestroy(h->ev_tail[x]); if (h->ev_qb[x]) (void)hipEventDestroy(h->ev_qb[x]); if (h->ev_fin[x]) (void)hipEventDestroy(h->ev_fin[x]); }
    if (h->h_msg) (void)hipHostFree(h->h_msg);
    if (h->h_tmp) (void)hipHostFree(h->h_tmp);
    if (h->red_mem) (void)hipHostFree(h->red_mem);
    if (h->shm) { shm_close(h->shm); delete h->shm; }
    if (h->h_abort) (void)hipHostFree(h->h_abort);
    if (!h->P.slot_dev) {                   // device slots are in allocs
        if (h->P.hidx) (void)hipHostFree(h->P.hidx);
        if (h->P.hval) (void)hipHostFree(h->P.hval);
        if (h->P.hreq) (void)hipHostFree(h->P.hreq);
    }
    for (auto &e : h->evpool) (void)hipEventDestroy(e);
    for (auto &e : h->op_ev) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// ---- transports between the GPUs of one job ---------------------------------------------------------
extern "C" int ttx_comm_unique_id(uint8_t id[128])
{
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId u;
    NCCLCHECK(g_rccl.GetUniqueId(&u));
    memcpy(id, u.internal, 128);
    return TTX_OK;
}
extern "C" int ttx_comm_init(ttx_engine *h, const uint8_t id[128])
{
    if (!h) return fail(TTX_EINVAL, "ttx_comm_init: null handle");
    if (h->cfg.fun_id == TTX_FUN_TRAINS) return fail(TTX_ESTATE, "ttx_comm_init: an engine with an integrand of trains (TTX_FUN_TRAINS) runs in one process");
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) return fail(TTX_ESTATE, "ttx_comm_init: an engine with a pulled-back integrand (TTX_FUN_PULLBACK) runs in one process");
    if (h->W == 1) return TTX_OK;
    int rc = rccl_load();
    if (rc) return rc;
    HIPCHECK(hipSetDevice(h->cfg.device));
    ncclUniqueId u;
    memcpy(u.internal, id, 128);
    NCCLCHECK(g_rccl.CommInitRank(&h->comm, h->W, u, h->wrank));
    return TTX_OK;
}
// Loop-back self-test of the RCCL transport on ONE device: a communicator of one rank, then exactly the calls the multi-GPU data
// path makes -- a grouped ncclSend / ncclRecv pair of one packed neighbour message (ncclChar) on a non-blocking stream, the
// 3-double MAX all-reduce of the sweep maxima and a SUM all-reduce of doubles (quadrature partials / per-sweep summary) -- each
// followed by a byte comparison.  It exercises the dlopen'ed symbol table, the datatypes and the stream ordering on pools where
// a second GPU (and with it ttx_comm_init with world_size > 1) is not available.
extern "C" int ttx_k_rccl_selftest(int32_t device, int64_t msg_bytes, int32_t nsum)
{
    if (msg_bytes < 1 || nsum < 1) return fail(TTX_EINVAL, "ttx_k_rccl_selftest: bad sizes");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(TTX_ENODEV, "no HIP device");
    HIPCHECK(hipSetDevice(device));
    int rc = rccl_load();
    if (rc) return rc;
    ncclUniqueId u;
    NCCLCHECK(g_rccl.GetUniqueId(&u));
    ncclComm_t comm = nullptr;
    NCCLCHECK(g_rccl.CommInitRank(&comm, 1, u, 0));
    hipStream_t st = nullptr;
    char *dsend = nullptr, *drecv = nullptr; double *dred = nullptr, *dout = nullptr;
    std::vector<char> hs((size_t)msg_bytes), hr((size_t)msg_bytes);
    std::vector<double> hd((size_t)nsum + 4), ho((size_t)nsum + 4);
    for (int64_t i = 0; i < msg_bytes; i++) hs[(size_t)i] = (char)((i * 131 + 7) & 0xff);
    for (size_t i = 0; i < hd.size(); i++) hd[i] = 1.0 / (double)(i + 3) - 0.25 * (double)(i % 5);
    int bad = 0;
    auto body = [&]() -> int {
        HIPCHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        HIPCHECK(hipMalloc((void **)&dsend, (size_t)msg_bytes)); HIPCHECK(hipMalloc((void **)&drecv, (size_t)msg_bytes));
        HIPCHECK(hipMalloc((void **)&dred, sizeof(double) * hd.size())); HIPCHECK(hipMalloc((void **)&dout, sizeof(double) * hd.size()));
        HIPCHECK(hipMemcpyAsync(dsend, hs.data(), (size_t)msg_bytes, hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemsetAsync(drecv, 0, (size_t)msg_bytes, st));
        HIPCHECK(hipMemcpyAsync(dred, hd.data(), sizeof(double) * hd.size(), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemsetAsync(dout, 0, sizeof(double) * hd.size(), st));
        NCCLCHECK(g_rccl.GroupStart());
        NCCLCHECK(g_rccl.Send(dsend, (size_t)msg_bytes, ncclChar, 0, comm, st));
        NCCLCHECK(g_rccl.Recv(drecv, (size_t)msg_bytes, ncclChar, 0, comm, st));
        NCCLCHECK(g_rccl.GroupEnd());
        NCCLCHECK(g_rccl.AllReduce(dred, dout, 4, ncclDouble, ncclMax, comm, st));                          // amax, pivotmax, -pivotmin (+ pad)
        NCCLCHECK(g_rccl.AllReduce(dred + 4, dout + 4, (size_t)nsum, ncclDouble, ncclSum, comm, st));        // summary / quadrature partials
        HIPCHECK(hipMemcpyAsync(hr.data(), drecv, (size_t)msg_bytes, hipMemcpyDeviceToHost, st));
        HIPCHECK(hipMemcpyAsync(ho.data(), dout, sizeof(double) * ho.size(), hipMemcpyDeviceToHost, st));
        HIPCHECK(hipStreamSynchronize(st));
        if (memcmp(hs.data(), hr.data(), (size_t)msg_bytes) != 0) bad |= 1;
        if (memcmp(hd.data(), ho.data(), sizeof(double) * hd.size()) != 0) bad |= 2;
        return TTX_OK;
    };
    rc = body();
    if (dsend) (void)hipFree(dsend); if (drecv) (void)hipFree(drecv); if (dred) (void)hipFree(dred); if (dout) (void)hipFree(dout);
    if (st) (void)hipStreamDestroy(st);
    (void)g_rccl.CommDestroy(comm);
    if (rc) return rc;
    if (bad) return fail(TTX_EHIP, "ttx_k_rccl_selftest: %s came back different", bad == 1 ? "the point-to-point message" : bad == 2 ? "an all-reduce" : "message and all-reduce");
    return TTX_OK;
}

// ---- built-in node-local host transport over POSIX shared memory (ttx_shm.h) -----------------------------------------
extern "C" int ttx_comm_init_shm(ttx_engine *h, const char *name)
{
    if (!h || !name || !*name) return fail(TTX_EINVAL, "ttx_comm_init_shm: null argument");
    if (h->cfg.fun_id == TTX_FUN_TRAINS) return fail(TTX_ESTATE, "ttx_comm_init_shm: an engine with an integrand of trains (TTX_FUN_TRAINS) runs in one process");
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) return fail(TTX_ESTATE, "ttx_comm_init_shm: an engine with a pulled-back integrand (TTX_FUN_PULLBACK) runs in one process");
    if (h->W == 1) return TTX_OK;
    if (h->shm) return fail(TTX_ESTATE, "ttx_comm_init_shm: already initialised");
    ShmTransport *T = new ShmTransport();
    std::string text;
    if (int rc = shm_attach(name, h->wrank, h->W, (h->P.MSZ + 63) & ~(size_t)63, std::max<size_t>(std::max(h->QB, h->SB), 8), T, &text)) {
        delete T;
        return fail(rc, "%s", text.c_str());
    }
    h->shm = T;
    h->cb.ctx = T; h->cb.sendrecv = shm_sendrecv; h->cb.allreduce = shm_allreduce; h->have_cb = true;
    // everybody is attached before rank 0 may unlink the name at destroy time
    if (shm_barrier(T)) return fail(TTX_EHIP, "ttx_comm_init_shm: not all %d ranks attached", T->W);
    return TTX_OK;
}

extern "C" int ttx_set_transport(ttx_engine *h, const ttx_transport *t)
{
    if (!h || !t || !t->sendrecv || !t->allreduce) return fail(TTX_EINVAL, "ttx_set_transport: null argument");
    if (h->cfg.fun_id == TTX_FUN_TRAINS) return fail(TTX_ESTATE, "ttx_set_transport: an engine with an integrand of trains (TTX_FUN_TRAINS) runs in one process");
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) return fail(TTX_ESTATE, "ttx_set_transport: an engine with a pulled-back integrand (TTX_FUN_PULLBACK) runs in one process");
    h->cb = *t; h->have_cb = true;
    return TTX_OK;
}

extern "C" int ttx_set_integrand_host(ttx_engine *h, ttx_host_fun fun, const double *par)
{
    if (!h || !fun) return fail(TTX_EINVAL, "ttx_set_integrand_host: null argument");
    if (h->cfg.fun_id != TTX_FUN_HOST) return fail(TTX_ESTATE, "ttx_set_integrand_host: the engine was not created with fun_id = TTX_FUN_HOST");
    h->hfun = fun; h->hfun_par = par;
    return TTX_OK;
}
extern "C" int64_t ttx_host_calls(const ttx_engine *h) { return h ? h->host_calls : 0; }

// a code object into a DevFun: the module, the three symbols <prefix>{info,slots,list}_<name>, the device copy of par.  `who` names
// the entry in the messages, `macro` the header macro that generates the symbols.  Nothing of the engine changes here.
static int devfun_load(const char *who, const char *prefix, const char *macro, const char *what, ttx_engine *h, const void *image, int64_t nbytes, const char *name,
                       const double *par, int32_t npar, std::shared_ptr<DevFun> *out)
{
    if (!image || nbytes <= 0) return fail(TTX_EINVAL, "%s: empty code object image", who);
    if (!name || !*name || strlen(name) > 200) return fail(TTX_EINVAL, "%s: integrand name missing (or longer than 200 characters)", who);
    if (npar < 0 || (npar > 0 && !par)) return fail(TTX_EINVAL, "%s: par missing (npar = %d)", who, npar);
    if (!devfun_image_plausible((const unsigned char *)image, (size_t)nbytes))
        return fail(TTX_EINVAL, "%s: the image is neither a complete code object (ELF) nor a complete offload bundle of hipcc --genco", who);
    HIPCHECK(hipSetDevice(h->cfg.device));
    // the runtime may keep pointers into the image: the loader gets a private copy that lives as long as the module
    auto f = std::make_shared<DevFun>();
    f->device = h->cfg.device; f->name = name;
    f->image.assign((const unsigned char *)image, (const unsigned char *)image + nbytes);
    f->image.push_back(0);
    hipError_t e = hipModuleLoadData(&f->mod, f->image.data());
    if (e != hipSuccess) {
        (void)hipGetLastError(); f->mod = nullptr;
        return fail(TTX_EINVAL, "%s: the runtime refused the code object (%s): is it built for this GPU (--offload-arch=gfx950)?", who, hipGetErrorString(e));
    }
    const std::string sn = std::string(prefix) + "slots_" + name, ln = std::string(prefix) + "list_" + name, in = std::string(prefix) + "info_" + name;
    hipDeviceptr_t ip = nullptr; size_t ib = 0;
    if ((e = hipModuleGetGlobal(&ip, &ib, f->mod, in.c_str())) != hipSuccess || hipModuleGetFunction(&f->slots, f->mod, sn.c_str()) != hipSuccess ||
        hipModuleGetFunction(&f->list, f->mod, ln.c_str()) != hipSuccess) {
        (void)hipGetLastError();
        return fail(TTX_EINVAL, "%s: the code object has no %s '%s' (symbols %s, %s, %s: see %s in ttx_device_fun.h)",
                    who, what, name, in.c_str(), sn.c_str(), ln.c_str(), macro);
    }
    if (ib < sizeof(int)) return fail(TTX_EINVAL, "%s: %s is not a ttx_devfun_info", who, in.c_str());
    HIPCHECK(hipMemcpy(&f->info, (const void *)ip, std::min(ib, sizeof(f->info)), hipMemcpyDeviceToHost));
    if (f->info.abi != TTX_DEVFUN_ABI || ib != sizeof(f->info))
        return fail(TTX_EINVAL, "%s: integrand '%s' was compiled against slot ABI version %d, this engine speaks version %d: recompile it with this engine's ttx_device_fun.h",
                    who, name, f->info.abi, TTX_DEVFUN_ABI);
    if ((f->info.kind != TTX_DEVFUN_KIND_LANE && f->info.kind != TTX_DEVFUN_KIND_WAVE) || f->info.block < 64 || f->info.block > 1024 || f->info.block % 64)
        return fail(TTX_EINVAL, "%s: integrand '%s': bad kind / block size (%d / %d)", who, name, f->info.kind, f->info.block);
    const long long lds = (long long)f->info.lds_per_wave * (f->info.block / 64);
    if (f->info.lds_per_wave < 0 || lds > 64 * 1024)
        return fail(TTX_EINVAL, "%s: integrand '%s' asks for %lld bytes of LDS per workgroup (%d per wave), more than 64 KB", who, name, lds, f->info.lds_per_wave);
    HIPCHECK(hipMalloc((void **)&f->par, sizeof(double) * (size_t)(npar + 1)));
    if (npar > 0) HIPCHECK(hipMemcpy(f->par, par, sizeof(double) * (size_t)npar, hipMemcpyHostToDevice));
    *out = std::move(f);
    return TTX_OK;
}
extern "C" int ttx_set_integrand_device(ttx_engine *h, const void *image, int64_t nbytes, const char *name, const double *par, int32_t npar)
{
    if (!h) return fail(TTX_EINVAL, "ttx_set_integrand_device: null handle");
    if (h->cfg.fun_id != TTX_FUN_DEVICE) return fail(TTX_ESTATE, "ttx_set_integrand_device: the engine was not created with fun_id = TTX_FUN_DEVICE");
    std::shared_ptr<DevFun> f;
    if (int rc = devfun_load("ttx_set_integrand_device", "ttx_devfun_", "TTX_DEVICE_INTEGRAND", "integrand", h, image, nbytes, name, par, npar, &f)) return rc;
    HIPCHECK(hipStreamSynchronize(h->stream));          // nothing of an earlier integrand is in flight when its module goes
    h->dfun = std::move(f);
    return TTX_OK;
}
extern "C" int ttx_set_integrand_device_file(ttx_engine *h, const char *path, const char *name, const double *par, int32_t npar)
{
    if (!h) return fail(TTX_EINVAL, "ttx_set_integrand_device_file: null handle");
    if (h->cfg.fun_id != TTX_FUN_DEVICE) return fail(TTX_ESTATE, "ttx_set_integrand_device_file: the engine was not created with fun_id = TTX_FUN_DEVICE");
    std::vector<unsigned char> buf;
    std::string text;
    if (int rc = devfun_read_file("ttx_set_integrand_device_file", path, buf, &text)) return fail(rc, "%s", text.c_str());
    return ttx_set_integrand_device(h, buf.data(), (int64_t)buf.size(), name, par, npar);
}
// the loaded integrand at a list of multi-indices, through the code object's list kernel
extern "C" int ttx_eval_device(ttx_engine *h, int64_t npts, const int32_t *ind, double *out)
{
    if (!h) return fail(TTX_EINVAL, "ttx_eval_device: null handle");
    if (h->cfg.fun_id == TTX_FUN_TRAINS) return tf_eval_list(h, npts, ind, out);
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) return pb_eval_list(h, npts, ind, out);
    if (h->cfg.fun_id != TTX_FUN_DEVICE) return fail(TTX_ESTATE, "ttx_eval_device: the engine was not created with fun_id = TTX_FUN_DEVICE");
    if (!h->dfun) return fail(TTX_ESTATE, "ttx_eval_device: call ttx_set_integrand_device first");
    if (npts < 0 || (npts > 0 && (!ind || !out))) return fail(TTX_EINVAL, "ttx_eval_device: null argument");
    if (npts == 0) return TTX_OK;
    int d = h->d;
    for (int64_t p = 0; p < npts; p++)
        for (int k = 0; k < d; k++)
            if (ind[p * d + k] < 1 || ind[p * d + k] > h->n1[k + 1])
                return fail(TTX_EINVAL, "ttx_eval_device: point %lld: index %d of mode %d is outside 1..%d", (long long)p, ind[p * d + k], k + 1, h->n1[k + 1]);
    HIPCHECK(hipSetDevice(h->cfg.device));
    DevFun &f = *h->dfun;
    int *dind = nullptr; double *dout = nullptr;
    HIPCHECK(hipMalloc((void **)&dind, sizeof(int) * (size_t)npts * d));
    if (hipMalloc((void **)&dout, sizeof(double) * (size_t)npts) != hipSuccess) { (void)hipFree(dind); return fail(TTX_EHIP, "ttx_eval_device: out of device memory"); }
    int rc = TTX_OK;
    long long np = npts;
    const int *n = h->P.n + 1;
    const double *par = f.par;
    const int waves = f.info.block / 64;
    const long long want = f.info.kind == TTX_DEVFUN_KIND_WAVE ? (np + waves - 1) / waves : (np + f.info.block - 1) / f.info.block;
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(want, 4096));
    void *args[] = {&d, &n, &par, &np, &dind, &dout};
    hipError_t e = hipMemcpyAsync(dind, ind, sizeof(int) * (size_t)npts * d, hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipModuleLaunchKernel(f.list, grid, 1, 1, (unsigned)f.info.block, 1, 1, (unsigned)(f.info.lds_per_wave * waves), h->stream, args, nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, sizeof(double) * (size_t)npts, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) rc = fail(TTX_EHIP, "ttx_eval_device: %s", hipGetErrorString(e));
    (void)hipFree(dind); (void)hipFree(dout);
    return rc;
}

// host functions of the stream-ordered host transport (run on a runtime thread when the stream reaches them; no HIP calls)
static void hostfn_xfer(void *ud)
{
    ttx_engine *h = (ttx_engine *)ud;
    const DevProb &P = h->P;
    const int left = (h->g0 > 0) ? h->wrank - 1 : -1, right = (h->g0 + h->G < h->cfg.nproc) ? h->wrank + 1 : -1;
    char *sR = h->h_msg, *sL = h->h_msg + P.MSZ, *rL = h->h_msg + 2 * P.MSZ, *rR = h->h_msg + 3 * P.MSZ;
    if (h->cb.sendrecv(h->cb.ctx, right, sR, (int64_t)P.MSZ, left, rL, (int64_t)P.MSZ)) h->cb_error = 1;
    if (h->cb.sendrecv(h->cb.ctx, left, sL, (int64_t)P.MSZ, right, rR, (int64_t)P.MSZ)) h->cb_error = 1;
}
static void hostfn_allreduce(void *ud)
{
    ttx_engine::RedJob *j = (ttx_engine::RedJob *)ud;
    if (j->h->cb.allreduce(j->h->cb.ctx, j->buf, (int64_t)j->count, j->op)) j->h->cb_error = 1;
}

// messages of the boundary groups to the neighbouring GPUs (device buffers; after k_exch_pack)
static int xfer_neighbours(ttx_engine *h)
{
    if (h->W == 1) return TTX_OK;
    DevProb &P = h->P;
    const int left = (h->g0 > 0) ? h->wrank - 1 : -1, right = (h->g0 + h->G < h->cfg.nproc) ? h->wrank + 1 : -1;
    char *outR = P.msgR + (size_t)(h->G - 1) * P.MSZ, *outL = P.msgL;
    if (h->comm) {
        NCCLCHECK(g_rccl.GroupStart());
        if (right >= 0) { NCCLCHECK(g_rccl.Send(outR, P.MSZ, ncclChar, right, h->comm, h->stream)); NCCLCHECK(g_rccl.Recv(h->recvR, P.MSZ, ncclChar, right, h->comm, h->stream)); }
        if (left >= 0) { NCCLCHECK(g_rccl.Send(outL, P.MSZ, ncclChar, left, h->comm, h->stream)); NCCLCHECK(g_rccl.Recv(h->recvL, P.MSZ, ncclChar, left, h->comm, h->stream)); }
        NCCLCHECK(g_rccl.GroupEnd());
        return TTX_OK;
    }
    if (!h->have_cb) return fail(TTX_ESTATE, "world_size > 1 but neither ttx_comm_init nor ttx_set_transport was called");
    // Host transport, STREAM-ORDERED: device -> pinned copies, then a host function enqueued in the stream runs the two
    // sendrecv calls, then pinned -> device copies.  The host thread that called ttx_run does not wait: the control flow
    // (and therefore the pipelined sweep loop) is the same as with RCCL, only the primitive differs.
    char *sR = h->h_msg, *sL = h->h_msg + P.MSZ;
    if (right >= 0) HIPCHECK(hipMemcpyAsync(sR, outR, P.MSZ, hipMemcpyDeviceToHost, h->stream));
    if (left >= 0) HIPCHECK(hipMemcpyAsync(sL, outL, P.MSZ, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipLaunchHostFunc(h->stream, hostfn_xfer, h));
    if (left >= 0) HIPCHECK(hipMemcpyAsync(h->recvL, h->h_msg + 2 * P.MSZ, P.MSZ, hipMemcpyHostToDevice, h->stream));
    if (right >= 0) HIPCHECK(hipMemcpyAsync(h->recvR, h->h_msg + 3 * P.MSZ, P.MSZ, hipMemcpyHostToDevice, h->stream));
    return TTX_OK;
}
// all-reduce of `count` doubles from device buffer src into device buffer dst; op 0 = sum, 1 = max
static int allreduce_dev(ttx_engine *h, const double *src, double *dst, size_t count, int op)
{
    if (h->W == 1) return TTX_OK;                       // dst aliases src
    if (h->comm) { NCCLCHECK(g_rccl.AllReduce(src, dst, count, ncclDouble, op ? ncclMax : ncclSum, h->comm, h->stream)); return TTX_OK; }
    if (!h->have_cb) return fail(TTX_ESTATE, "world_size > 1 but neither ttx_comm_init nor ttx_set_transport was called");
    // each pending reduction gets its own pinned slot and descriptor (several may be enqueued before the first one runs)
    ttx_engine::RedJob *job = h->red_slot(count, op);
    if (!job) return fail(TTX_EHIP, "allreduce staging exhausted");
    HIPCHECK(hipMemcpyAsync(job->buf, src, sizeof(double) * count, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipLaunchHostFunc(h->stream, hostfn_allreduce, job));
    HIPCHECK(hipMemcpyAsync(dst, job->buf, sizeof(double) * count, hipMemcpyHostToDevice, h->stream));
    return TTX_OK;
}

// ---- launch helpers -------------------------------------------------------------------------------
static hipEvent_t ev_get(ttx_engine *h)
{
    if (!h->evpool.empty()) { hipEvent_t e = h->evpool.back(); h->evpool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
// brackets `n` consecutive launches of one kind with a single HIP event pair on the engine's stream
struct KScope {
    ttx_engine *h; int kind, n; hipEvent_t a = nullptr, b = nullptr;
    KScope(ttx_engine *h_, int kind_, int n_ = 1) : h(h_), kind(kind_), n(n_) { if (h->profile) { a = ev_get(h); b = ev_get(h); (void)hipEventRecord(a, h->stream); } }
    ~KScope() { if (h->profile) { (void)hipEventRecord(b, h->stream); h->evs.push_back({kind, n, a, b}); } else h->k_launches[kind] += n; }
};
static void ev_collect(ttx_engine *h)
{
    for (auto &e : h->evs) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, e.a, e.b);
        h->k_ms[e.kind] += ms; h->k_launches[e.kind] += e.n;
        h->evpool.push_back(e.a); h->evpool.push_back(e.b);
    }
    h->evs.clear();
}

static double erank_host(const ttx_engine *h, const int32_t *r)
{
    // lib/tt.f90:1228-1245
    const int l = 1, m = h->d, d = m;
    if (d == 1) return 0.0;
    double s = 0.0;
    for (int i = l; i <= m; i++) s = s + r[i - 1] * h->n1[i] * r[i];
    if (s == 0.0) return s;
    int b = r[l - 1] * h->n1[l] + h->n1[m] * r[m];
    if (d == 2) return s / b;
    int a = 0;
    for (int i = l + 1; i <= m - 1; i++) a += h->n1[i];
    return (std::sqrt(b * b + 4.0 * a * s) - b) / (2.0 * a);
}

// Fortran Ew.d (the optional leading zero is dropped when the sign needs its place)
static std::string fmt_e(int w, int dgt, double v)
{
    char tmp[64], body[64];
    if (v != 0.0 && std::isfinite(v)) {
        snprintf(tmp, sizeof tmp, "%.*e", dgt - 1, v);
        char *e = strchr(tmp, 'e');
        int ex = atoi(e + 1) + 1;
        *e = 0;
        std::string digs;
        for (char *c = tmp; *c; c++) if (*c >= '0' && *c <= '9') digs.push_back(*c);
        snprintf(body, sizeof body, ".%sE%c%02d", digs.c_str(), ex < 0 ? '-' : '+', abs(ex));
    } else snprintf(body, sizeof body, ".%sE+00", std::string(dgt, '0').c_str());
    std::string s = body;
    const bool neg = std::signbit(v) && v != 0.0;
    if ((int)s.size() + 1 + (neg ? 1 : 0) <= w) s = "0" + s;
    if (neg) s = "-" + s;
    if ((int)s.size() < w) s = std::string(w - s.size(), ' ') + s;
    return s;
}

static void print_line(const ttx_engine *h, const ttx_sweep_rec &r, double val_prev)
{
    // lib/dmrgg.f90:971-1008 (printed by rank 0 only)
    if (h->wrank != 0) return;
    const char *sd = r.dir == 0 ? "::" : r.dir == 1 ? ">>" : "<<";
    printf("%3d%2s rank%5.1f time: %s n_evals: %10lld", r.it, sd, r.erank, fmt_e(9, 3, r.seconds).c_str(), (long long)r.neval);
    if (h->P.has_quad) {
        if (r.it == 0) printf(" val %s", fmt_e(20, 14, r.val).c_str());
        else if (h->cfg.has_tru) printf(" err %s val %s", fmt_e(8, 3, std::fabs(1.0 - r.val / h->cfg.tru)).c_str(), fmt_e(20, 14, r.val).c_str());
        else printf(" cnv %s val %s", fmt_e(8, 3, std::fabs(1.0 - r.val / val_prev)).c_str(), fmt_e(20, 14, r.val).c_str());
    }
    printf("\n");
    fflush(stdout);
}

// job-wide summary of the sweep -> h->h_sum (one all-reduce, one stream synchronisation)
// in two halves, so that the end of a pipelined run can enqueue the first one ahead of its other waits (LoopPlan::fin_early: one
// process, where the all-reduce is empty, on the quadrature's stream sq)
static int readback_enqueue(ttx_engine *h, double *dst, hipStream_t sq)
{
    hipLaunchKernelGGL(k_collect, dim3(1), dim3(256), 0, sq, h->P);
    int rc = allreduce_dev(h, h->P.sumsend, h->P.sumrecv, h->SB, 0);
    if (rc) return rc;
    HIPCHECK(hipMemcpyAsync(dst, h->P.sumrecv, sizeof(double) * h->SB, hipMemcpyDeviceToHost, sq));
    return TTX_OK;
}
static int readback_wait(ttx_engine *h)
{
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (h->cb_error) return fail(TTX_EHIP, "host transport: a sendrecv / allreduce callback failed");
    if (h->profile) ev_collect(h);
    return TTX_OK;
}
static int readback(ttx_engine *h)
{
    if (int rc = readback_enqueue(h, h->h_sum, h->stream)) return rc;
    return readback_wait(h);
}
static inline const double *sum_bond(const ttx_engine *h, int p) { return h->h_sum + SUM_HDR + h->cfg.nproc + 5 * (size_t)p; }

// bond ranks as the owning groups hold them (valid after readback)
static std::vector<int32_t> global_ranks(const ttx_engine *h)
{
    std::vector<int32_t> r(h->d + 1, 1);
    for (int p = 1; p < h->d; p++) r[p] = (int32_t)sum_bond(h, p)[0];
    return r;
}
// The reference prints erank(arg) of rank 0, whose knowledge of a bond owned by rank g lags g-1 sweeps behind
// (the pivot tape hops one rank per sweep, lib/dmrgg.f90:768-850).  The engine ships pivots only to direct
// neighbours, so the lag is reproduced here from the per-sweep history of accepted pivots.
static std::vector<int32_t> rank0_view(ttx_engine *h, int it)
{
    const int d = h->d;
    if (it == 0) { h->updhist.clear(); return std::vector<int32_t>(d + 1, 1); }
    std::vector<uint8_t> u(d + 1, 0);
    for (int p = 1; p < d; p++) u[p] = sum_bond(h, p)[1] > 0.0;
    h->updhist.push_back(u);
    std::vector<int32_t> r(d + 1, 1);
    for (int g = 0; g < h->cfg.nproc; g++) {
        int lag = std::max(0, g - 1), upto = it - lag;       // sweeps 1..upto of group g's bonds are known to rank 0
        for (int p = h->own[g]; p < h->own[g + 1]; p++)
            for (int t = 1; t <= upto; t++) r[p] += h->updhist[t - 1][p];
    }
    return r;
}

// dynamic LDS of the kernels that update the persistent tables of the fast arithmetic next to their own work
static inline size_t lds_fpersist(const DevProb &P) { return (P.arith && P.fpersist) ? sizeof(double) * 4 * (P.d + 8) : 0; }

// quadrature of the cores as Q sees them, with the weights w, on the stream sq: per-core matrices, per-group chains, gather over
// GPUs, tree (the gather travels on the engine's stream: with several processes sq is that stream)
// built: recorded behind k_quad_build, the only kernel of the three that reads the cores
static int launch_quad(ttx_engine *h, hipStream_t sq, const DevProb &Q, int mode, const double *w, hipEvent_t built = nullptr)
{
    const size_t lds_q = sizeof(double) * ((size_t)h->RM * h->RM + 2);
    hipLaunchKernelGGL(k_quad_build, dim3(h->NC, h->G), dim3(256), lds_q, sq, Q, mode, w);
    if (built) HIPCHECK(hipEventRecord(built, sq));
    hipLaunchKernelGGL(k_quad_chain, dim3(h->G), dim3(256), Q.qscr ? 0 : 2 * lds_q, sq, Q);
    if (h->cfg.nproc > 1) {
        int rc = allreduce_dev(h, Q.qsend, Q.qall, h->QB, 0);
        if (rc) return rc;
        hipLaunchKernelGGL(k_quad_tree, dim3(1), dim3(256), h->sel.lds_qtree, sq, Q, h->sel.lds_qtree ? 1 : 0);
    }
    return TTX_OK;
}

// ---- the launch plan of the chain path -------------------------------------------------------------------------------------------
// One launch: the kernel, its source name with the template arguments that select behaviour (ttx_plan_describe), its shape, its
// dynamic LDS, and whether that LDS can exceed the default ceiling (the plan's builder then raises it, ensure_lds).
struct KLaunch {
    const void *fn = nullptr; const char *name = "-"; dim3 grid, block; size_t lds = 0; bool raise = false;
    explicit operator bool() const { return fn != nullptr; }
};
template <class F>
static KLaunch kl(F *fn, const char *name, dim3 grid, dim3 block, size_t lds, bool raise = false)
{
    KLaunch k; k.fn = reinterpret_cast<const void *>(fn); k.name = name; k.grid = grid; k.block = block; k.lds = lds; k.raise = raise;
    return k;
}
// the arguments exactly as the kernel declares them (a DevProb, then ints); like a <<< >>> launch, an error is left to the next hipGetLastError
template <class... A>
static void launch(hipStream_t st, const KLaunch &k, const A &...a)
{
    static_assert(((std::is_same<A, DevProb>::value || std::is_same<A, int>::value) && ...), "the chain kernels take a DevProb and ints");
    void *args[] = {(void *)&a...};
    (void)hipLaunchKernel(k.fn, k.grid, k.block, args, k.lds, st);
}
// What one run of the chain path launches per bond step, decided once from the engine's flags (chain_plan): the one place a kernel
// variant is wired in.  Built per run, because a fallback of ttx_run can retire the teams, the relay or the cluster path in between.
struct ChainPlan {
    KLaunch tables;                     // before the lottery: k_de_ctables, k_de_tables, k_fast_tables<FUN>, or none
    KLaunch lottery, lot_eval;          // one k_lottery<FUN> launch; with lot_eval: drawing launch, candidate evaluator, scoring launch
    int lot_vals = 0;
    struct Tier { KLaunch k; int upto = 0; };   // before the last tier: a grid of the sweep's units, taken while units * G <= upto
    Tier half[3]; int ntier = 0;        // the half-step: the first tier that applies; the last one always does
    int half_vals = -1;                 // the fifth argument of k_halfstep<FUN>; -1: the tiers' kernels take four
    KLaunch base; int base_vals = 0;    // k_halfstep<FUN>: full pivoting goes through it whatever the tiers are
    enum { FP_PLAIN, FP_MFMA, FP_COLUMNS } fullpiv = FP_PLAIN;      // piv = -1: all columns at once, dense MFMA, or one column per host pass
    KLaunch accept, init_samples, init_fibers, exch_boundary, fin_luar, fin_lual;
    KLaunch exch_tail;                  // not of the chain path: k_exch_tail<FUN> of the pipelined cluster loop, which shares exch_boundary's LDS figure
    int nfb = 0, srows = 0, fl = 0;
    std::vector<const KLaunch *> all() const
    {
        std::vector<const KLaunch *> v = {&tables, &lottery, &lot_eval, &base, &accept, &init_samples, &init_fibers, &exch_boundary, &exch_tail, &fin_luar, &fin_lual};
        for (int t = 0; t < ntier; t++) v.push_back(&half[t].k);
        return v;
    }
};
#define KFUN_(k) (FUN == FUN_ISING ? #k "<ISING>" : FUN == FUN_STDNORM ? #k "<STDNORM>" : FUN == FUN_MVN ? #k "<MVN>" : #k "<HOST>")
#define KUNIT_(k, ...) (P.de_unit ? kl(k<true>, #k "<true>", __VA_ARGS__) : kl(k<false>, #k "<false>", __VA_ARGS__))
#define KUNIT2_(k, x, ...) (P.de_unit ? kl(k<true, x>, #k "<true," #x ">", __VA_ARGS__) : kl(k<false, x>, #k "<false," #x ">", __VA_ARGS__))
template <int FUN>
static ChainPlan chain_plan(const ttx_engine *h)
{
    const DevProb &P = h->P;
    const CreatePlan &s = h->sel;
    const int d = h->d, G = h->G, RM = h->RM, NM = h->NM, nproc = h->cfg.nproc;
    const bool fastk = P.arith && (FUN == FUN_MVN || s.isDE);       // TTX_ARITH=fast with a re-associated evaluator (ttx_fast.h)
    const size_t VS = s.VS;
    ChainPlan p;
    p.nfb = s.nfb;
    p.base = kl(k_halfstep<FUN>, KFUN_(k_halfstep), dim3(p.nfb, G), dim3(TTX_BLK), s.lds_half, true);
    p.base_vals = fastk ? 0 : s.half_vals;
    p.lottery = kl(k_lottery<FUN>, "k_lottery", dim3(P.lot_nb, G), dim3(P.lot_nb == 1 ? 512 : 256), s.lds_lot, true);
    p.lot_vals = fastk ? s.fast_cap : s.lot_vals;
    // the Ising D/E kernels of ttx_de.h, by the division they use (de_unit: the short sequence for nodes in [0,1])
    const dim3 slots(s.de_slots, G), cand(P.lot_max, G), cand4((P.lot_max + 3) / 4, G);
    const KLaunch de = KUNIT_(k_halfstep_de, slots, dim3(64), s.lds_de, true);
    const KLaunch det3 = KUNIT2_(k_halfstep_det, 3, dim3(1, G), dim3(64 * 14), s.lds_det, true);
    const KLaunch det1 = KUNIT2_(k_halfstep_det, 1, dim3(1, G), dim3(64 * 6), s.lds_det6, true);
    const KLaunch de5 = KUNIT_(k_halfstep_de5, slots, dim3(64 * DE5_W), s.lds_de5, true);
    const KLaunch rows = KUNIT2_(k_lottery_eval_de_rows, false, cand4, dim3(64), s.lds_der, true);
    const KLaunch rows_tab = KUNIT2_(k_lottery_eval_de_rows, true, cand4, dim3(64), s.lds_der, true);
    // lottery candidates by one wave each between the drawing and the scoring launch: mvn; D/E with compact tables, row-parallel
    // without tables up to d = 160 (measured: 23 % less lottery time at D_64, even at D_256), from the tables beyond
    // (TTX_DE_LOT_POINT=0/1 forces one); D/E with full tables four candidates per wave (TTX_LOTTERY_ROWS=2: with the pivots' factor
    // tables, measured slower: HBM latency)
    if (fastk) p.lot_eval = KLaunch();
    else if (FUN == FUN_MVN && s.mvn_v2) p.lot_eval = kl(k_lottery_eval_mvn, "k_lottery_eval_mvn", cand, dim3(64), s.lds_mvn);
    else if (FUN == FUN_ISING && P.de_cut && s.de_v2 && s.lot_cand)
        p.lot_eval = s.de_lot_point ? kl(k_lottery_eval_decp, "k_lottery_eval_decp", cand, dim3(64), sizeof(double) * (2 * (size_t)(d + 64) + 2048), true)
                                    : kl(k_lottery_eval_dec, "k_lottery_eval_dec", cand, dim3(64), s.lds_de, true);
    else if (FUN == FUN_ISING && s.lot_wave) p.lot_eval = s.lot_rows == 2 ? rows_tab : rows;
    if (p.lot_eval) { p.lottery.grid = dim3(1, G); p.lottery.block = dim3(512); }
    // half-step.  D/E with full tables: while the ranks are small (at most it + 1 during sweep it) a unit gets a team of 14 waves on
    // a CU of its own, up to de_team6_units a team of 6 waves (three such teams fit a CU), beyond that one wave -- or a relay of four
    if (fastk) { p.half[p.ntier++].k = p.base; p.half_vals = 0; }
    else if (FUN == FUN_MVN && s.mvn_v2) p.half[p.ntier++].k = kl(k_halfstep_mvn, "k_halfstep_mvn", slots, dim3(64), s.lds_mvn);
    else if (FUN == FUN_ISING && s.de_v2) {
        if (h->de_team() && !h->de_v5()) { p.half[p.ntier++] = {det3, s.de_team_units}; p.half[p.ntier++] = {det1, s.de_team6_units}; }
        p.half[p.ntier++].k = h->de_v5() ? de5 : P.de_cut ? kl(k_halfstep_dec, "k_halfstep_dec", slots, dim3(64), s.lds_de, true) : de;
    } else { p.half[p.ntier++].k = p.base; p.half_vals = s.half_vals; }
    p.fullpiv = FUN == FUN_HOST ? ChainPlan::FP_COLUMNS : P.fp_mfma ? ChainPlan::FP_MFMA : ChainPlan::FP_PLAIN;
    // roles A/B of k_accept: x[RM]; C/D: the staged LU
    p.accept = kl(k_accept, "k_accept", dim3(2 * p.nfb + 2 * NM + 1, G), dim3(TTX_BLK), sizeof(double) * std::max<size_t>(RM + 2, (size_t)std::min<int>(RM, 64) * std::min<int>(RM, 64)));
    {   // initial samples: index rows in LDS where they fit
        const bool own_rows = FUN != FUN_HOST && !(FUN == FUN_ISING && P.arith && P.ising_id != 1);
        const InitSamplesPlan ip = init_samples_plan(s.lds_par, VS, h->d, (long)s.nn * s.snum, own_rows, s.init_wide);
        p.srows = ip.rows;
        p.init_samples = kl(k_init_samples<FUN>, KFUN_(k_init_samples), dim3(G), dim3(ip.threads), ip.lds, ip.rows != 0);
        p.init_fibers = kl(k_init_fibers<FUN>, KFUN_(k_init_fibers), dim3(h->NC, G), dim3(256), s.lds_par);
    }
    // before a bond step's lottery.  Ising D/E: pair factors of the bond that do not span it (shared by all elements through a pivot),
    // compact where the nodes allow the unit cut; TTX_ARITH=fast, mvn with TTX_FAST_PERSIST=0: the per-pivot tables of the bond step
    // (Ising D/E keeps its fast tables per bond)
    if (s.de_npair) p.tables = P.de_cut ? kl(k_de_ctables, "k_de_ctables", dim3(2 * RM, G), dim3(256), sizeof(double) * (size_t)(d + 2))
                                    : kl(k_de_tables, "k_de_tables", dim3((2 * (d + 1) * RM + 255) / 256, G), dim3(256), 0);
    else if (fastk && !P.fpersist) p.tables = kl(k_fast_tables<FUN>, KFUN_(k_fast_tables), dim3(2 * RM, G), dim3(64), sizeof(double) * 2 * (d + 8));
    if (nproc > 1) {    // boundary corners; D/E: two value rows; mvn: 3 d + 1 doubles
        const size_t lds_b = s.lds_par + 16 + sizeof(short) * 2 * VS + sizeof(double) * (64 * 64 + 4) +
                             (P.bnd_wave ? sizeof(double) * (std::max<size_t>(2 * (size_t)de_rows_stride(d), 3 * (size_t)d + 2) + 8 + (P.de_cut ? 64 * 32 : 0)) : 0);
        p.exch_boundary = kl(k_exch_boundary<FUN>, KFUN_(k_exch_boundary), dim3(2 * NM, G), dim3(TTX_BLK), lds_b, true);
        // the same blocks plus one apply block per group, which may stage the persistent fast tables
        if constexpr (FUN != FUN_HOST) p.exch_tail = kl(k_exch_tail<FUN>, KFUN_(k_exch_tail), dim3(2 * NM + 1, G), dim3(TTX_BLK), std::max(lds_b, lds_fpersist(P)), true);
    }
    {   // finalisation.  Threads (= columns) per workgroup: as many as fit the LDS next to the LU panel (256, 128 or 64); the columns
        // of a core are spread over grid.z (at maxrank 64 the 256-thread staging did not fit: the kernels then ran out of L2 with one
        // workgroup per core, 6 ms at D_256)
        int ft = 256;
        while (ft > 64 && sizeof(double) * ((size_t)RM * RM + (size_t)ft * RM) > TTX_LDS_FIN) ft >>= 1;
        const size_t lds_f = sizeof(double) * ((size_t)RM * RM + (size_t)ft * RM);
        p.fl = lds_f <= TTX_LDS_WORK ? 1 : 0;
        const dim3 gr(h->NC, G, std::max(1, std::min(64, (NM * RM + ft - 1) / ft)));
        p.fin_luar = kl(k_fin_luar, "k_fin_luar", gr, dim3(ft), p.fl ? lds_f : 0, p.fl != 0);
        p.fin_lual = kl(k_fin_lual, "k_fin_lual", gr, dim3(ft), p.fl ? lds_f : 0, p.fl != 0);
    }
    return p;
}
#undef KFUN_
#undef KUNIT_
#undef KUNIT2_

#ifdef TTX_STAMPS   // debug build, after a run: the cycle stamps the kernels left
static int dump_stamps(ttx_engine *h)
{
    const DevProb &P = h->P;
    if (P.dbg) {   // per-wave cycle stamps of one bond step of the cluster kernel (WST in ttx_cluster.h), relative to the earliest one
        std::vector<long long> hb(8 * 64 * 8);
        HIPCHECK(hipMemcpy(hb.data(), P.dbg, sizeof(long long) * hb.size(), hipMemcpyDeviceToHost));
        long long t0 = 0;
        for (long long v : hb) if (v && (!t0 || v < t0)) t0 = v;
        for (int hh = 0; hh < 8; hh++) {
            bool any = false;
            for (int w = 0; w < 64; w++) if (hb[((size_t)hh * 64 + w) * 8]) any = true;
            if (!any) continue;
            fprintf(stderr, "half-step %d (cycles since the first stamp; per wave: start eval-done reduced published polled reduced2)\n", hh);
            for (int w = 0; w < 64; w++) {
                const long long *e = &hb[((size_t)hh * 64 + w) * 8];
                if (!e[0]) continue;
                fprintf(stderr, "  blk %d wave %d: %7lld %7lld %7lld %7lld %7lld %7lld\n", w / 4, w % 4, e[0] - t0, e[1] - t0, e[2] - t0, e[3] - t0, e[4] - t0, e[5] - t0);
            }
        }
    }
    // average wall_clock64 ticks (10 ns) per phase of the lottery (0) and half-step (1) kernels
    GroupState g0s;
    HIPCHECK(hipMemcpy(&g0s, P.gs, sizeof(GroupState), hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; k++) {
        fprintf(stderr, "stamps kernel %d (n=%lld):", k, g0s.nstamp[k]);
        for (int x = 0; x < 16; x++) fprintf(stderr, " %.2fus", g0s.nstamp[k] ? 0.01 * (double)g0s.stamp[k][x] / (double)g0s.nstamp[k] : 0.0);
        fprintf(stderr, "\n");
    }
    return TTX_OK;
}
#endif

// ---- the sweep driver: the host side of one dtt_dmrgg run ----------------------------------------------------------------------
// The form of the loop (L, ttx_loop_plan.h: the reasons stand there) and what the chain path launches (plan) are decided once; the
// steps read both.  Sweep it_ runs in direction 2 - it_ % 2; its summary, its value and their events use the pinned slot it_ & 1.
template <int FUN>
struct SweepRun {
    using clk = std::chrono::steady_clock;
    ttx_engine *const h; DevProb &P; const hipStream_t st;
    const int d, G, nproc, cluster, fused;      // cluster, fused: the whole-sweep kernel this run uses, if any
    const clk::time_point t0 = clk::now();
    LoopPlan L; ChainPlan plan;
    DevProb Pq;                                 // what the per-sweep quadrature sees: in the pipelined loop the snapshot of the ranks
    double val = 1.0, val_prev = 1.0;
    int strike = 0, sweeps = 0; bool ready = false, fin_enqueued = false;
    double *sum_final = nullptr;                // where the final summary was enqueued to ahead of the run's end (LoopPlan::fin_early)
    explicit SweepRun(ttx_engine *h_) : h(h_), P(h_->P), st(h_->stream), d(h_->d), G(h_->G), nproc(h_->cfg.nproc), cluster(h_->cluster_nb()), fused(h_->sel.fused) {}
    double since() const { return std::chrono::duration<double>(clk::now() - t0).count(); }
    // an evaluating kernel: once with the device integrand; with a host integrand twice around the host's calls
    template <class... A>
    int EV(const KLaunch &k, A... a)
    {
        if (FUN != FUN_HOST) { launch(st, k, P, a...); return TTX_OK; }
        DevProb Q = P;
        Q.hostpass = 1; launch(st, k, Q, a...);
        if (int rc = slot_eval(h)) return rc;
        Q.hostpass = 2; launch(st, k, Q, a...);
        return TTX_OK;
    }
    // the two plans of the run (the kernels of the chain path, and the whole-sweep kernel where one is used, may stage more than the
    // default 64 KB of dynamic LDS, 160 KB per CU on gfx950), reset (lib/dmrgg.f90:96-100, 141-148, 279-288), initial cross (:151-301)
    int prepare()
    {
        LoopIn in;
        in.whole = cluster || fused; in.cluster = cluster != 0; in.profile = h->profile; in.pipeline_off = env_off("TTX_PIPELINE");
        in.W = h->W; in.nproc = nproc; in.has_quad = P.has_quad; in.host_pass = FUN == FUN_HOST;
        in.sweep_tail = h->sel.sweep_tail; in.sweep_tail_side = h->sel.sweep_tail_side; in.maxrank = h->cfg.maxrank;
        in.head_direct = h->sel.head_direct; in.fin_early = h->sel.fin_early; in.fin_skip_exch = h->sel.fin_skip_exch;
        L = loop_plan(in);
        P.tail_side = L.side ? 1 : 0;
        h->recs.clear(); h->tapes.clear();
        plan = chain_plan<FUN>(h);
        for (const KLaunch *k : plan.all()) if (k->raise) if (int rc = ensure_lds(h, k->fn, k->lds)) return rc;
        if (fused) if (int rc = ensure_lds(h, reinterpret_cast<const void *>(k_sweep_fused), h->sel.lds_fused)) return rc;
        if (cluster) { if (int rc = ensure_lds_cluster(h)) return rc; *h->h_abort = 0; }
        Pq = P;
        if (L.pipe) Pq.r = P.rq;
        hipLaunchKernelGGL(k_reset, dim3(64), dim3(256), 0, st, P, h->SB, h->QB);
        {
            KScope ks(h, TTX_K_OTHER, 4);
            if (int rc = EV(plan.init_samples, h->sel.snum, h->sel.nn, FUN == FUN_HOST ? 0 : plan.srows, 0)) return rc;
            if (int rc = EV(plan.init_fibers)) return rc;
            hipLaunchKernelGGL(k_init_factors, dim3(h->NC, G), dim3(256), lds_fpersist(P), st, P);
            hipLaunchKernelGGL(k_init_final, dim3(G), dim3(256), 0, st, P, h->sel.init_wave ? 1 : 0, L.head_direct ? h->h_sum_base : (double *)nullptr);
        }
        if (L.head) {
            h->h_sum = h->h_sum_base;
            if (!L.head_direct) {
                hipLaunchKernelGGL(k_collect, dim3(1), dim3(256), 0, st, P);
                HIPCHECK(hipMemcpyAsync(h->h_sum, P.sumrecv, sizeof(double) * h->SB, hipMemcpyDeviceToHost, st));
            }
            HIPCHECK(hipEventRecord(h->ev_sum[0], st));
            if (int rc = launch_sweep_kernel(1)) return rc;
            HIPCHECK(hipEventSynchronize(h->ev_sum[0]));
        } else if (int rc = readback(h)) return rc;
        HIPCHECK(hipGetLastError());
        for (int g = 0; g < nproc; g++) val = (g == 0) ? h->h_sum[SUM_HDR + g] : val * h->h_sum[SUM_HDR + g];   // :259-267 PROD
        if (!P.has_quad) val = 0.0;
        val_prev = val;
        record(0, 0);
        ready = (1 >= h->cfg.maxrank);
        return TTX_OK;
    }
    // the one place that launches a whole-sweep kernel: behind the initial cross (L.head) and from both loops.  The cluster kernel can
    // go as a cooperative launch (TTX_CLUSTER_COOP: the runtime guarantees -- or refuses -- co-residency of the grid)
    int launch_sweep_kernel(int it_)
    {
        const CreatePlan &s = h->sel;
        int dir = 2 - it_ % 2, epoch = it_, nsteps = h->nbmax, NB = s.cluster, ldsinv = s.cluster_ldsinv;
        int zkeep = (s.cluster_zkeep ? CL_ZKEEP : 0) | (s.cl_lists ? CL_ZCARRY : 0) | (s.cl_word ? CL_WORD : 0) | (s.cl_powtab ? CL_POWTAB : 0)     // the forms of the entry
                    | (s.cl_pack2 ? CL_PACK2 : 0);      // ... and of the exit
        const dim3 grid(8 * NB * ((G + 7) / 8)), block(CB);
        KScope ks(h, TTX_K_HALFSTEP, 1);
        if (!cluster) hipLaunchKernelGGL(k_sweep_fused, dim3(G), dim3(FB), s.lds_fused, st, P, dir, nsteps);
        else if (s.cluster_coop) {
            void *args[] = {&P, &dir, &nsteps, &NB, &ldsinv, &epoch, &zkeep};
            HIPCHECK(hipLaunchCooperativeKernel(reinterpret_cast<const void *>(cluster_kernel(s.cluster_var)), grid, block, args, (unsigned)s.lds_cluster, st));
        } else hipLaunchKernelGGL(cluster_kernel(s.cluster_var), grid, block, s.lds_cluster, st, P, dir, nsteps, NB, ldsinv, epoch, zkeep);
        return TTX_OK;
    }
    // the chain path's sweep over the own bonds: tables, lottery, half-steps (or full pivoting), accept per bond step
    int enqueue_chain_sweep(int it_)
    {
        const int dir = 2 - it_ % 2;
        // the ranks are at most it_ + 1 in sweep it_: the units of a team half-step, and the columns of full pivoting by host passes
        const int rb = std::min((int)h->RM, it_ + 1);
        const int units = (h->sel.de_test_fault && it_ == h->sel.de_test_fault) ? 1 : rb * ((h->NM + 63) / 64);
        KLaunch half = plan.half[plan.ntier - 1].k;
        for (int t = plan.ntier - 2; t >= 0; t--) if (units * G <= plan.half[t].upto) { half = plan.half[t].k; half.grid.x = units; }
        for (int pp = 1; pp <= h->nbmax; pp++) {
            if (plan.tables) { KScope ks(h, TTX_K_OTHER); launch(st, plan.tables, P, dir, pp); }
            if (h->cfg.pivoting < 0) { if (int rc = enqueue_full_pivoting(dir, pp, rb)) return rc; }
            else {
                if (plan.lot_eval) {
                    KScope ks(h, TTX_K_LOTTERY, 3);
                    launch(st, plan.lottery, P, dir, pp, plan.lot_vals, 1);
                    launch(st, plan.lot_eval, P);
                    launch(st, plan.lottery, P, dir, pp, plan.lot_vals, 2);
                } else { KScope ks(h, TTX_K_LOTTERY); if (int rc = EV(plan.lottery, dir, pp, plan.lot_vals, 0)) return rc; }
                KScope ks(h, TTX_K_HALFSTEP, h->H);
                for (int hh = 0; hh < h->H; hh++) {
                    if (plan.half_vals < 0) launch(st, half, P, hh, dir, h->mode);
                    else if (int rc = EV(half, hh, dir, h->mode, plan.half_vals)) return rc;
                }
            }
            { KScope ks(h, TTX_K_ACCEPT); launch(st, plan.accept, P, h->H, plan.nfb); }
        }
        return TTX_OK;
    }
    // full pivoting (:341-408): every superblock column through the half-step kernel, global arg-max, then the cross through the
    // winner (evaluation only)
    int enqueue_full_pivoting(int dir, int pp, int rb)
    {
        KScope ks(h, TTX_K_HALFSTEP, 5);
        KLaunch cols = plan.base;
        cols.grid.z = h->NM * h->RM;
        hipLaunchKernelGGL(k_bond_begin, dim3(G), dim3(64), 0, st, P, dir, pp);
        if (plan.fullpiv == ChainPlan::FP_MFMA) {
            // one dense step: evaluate the superblock once, residual by fp64 MFMA fused with the arg-max
            const int side = h->RM * h->NM, gx = (side + 63) / 64;
            launch(st, cols, P, 0, dir, 4, plan.base_vals);
            hipLaunchKernelGGL(k_full_gemm_argmax, dim3(gx, gx, G), dim3(256), 0, st, P);
            hipLaunchKernelGGL(k_full_resolve2, dim3(G), dim3(256), 0, st, P, gx, gx);
        } else if (plan.fullpiv == ChainPlan::FP_COLUMNS) {
            // the user's `fun` with full pivoting (:341-408 works with any fun): one superblock column (k,q) per launch pair --
            // pass 1 hands the column's multi-indices to the host, pass 2 takes the values, residual and partial arg-max;
            // columns beyond n2 r2 return at once
            for (int z = 0; z < h->NM * rb; z++) {
                DevProb Q = P;
                Q.zbase = z;
                Q.hostpass = 1; launch(st, plan.base, Q, 0, dir, 3, 0);
                if (int rc = slot_eval(h)) return rc;
                Q.hostpass = 2; launch(st, plan.base, Q, 0, dir, 3, 0);
            }
            hipLaunchKernelGGL(k_full_resolve, dim3(G), dim3(256), 0, st, P);
        } else {
            launch(st, cols, P, 0, dir, 3, plan.base_vals);
            hipLaunchKernelGGL(k_full_resolve, dim3(G), dim3(256), 0, st, P);
        }
        if (int rc = EV(plan.base, 0, dir, 2, plan.base_vals)) return rc;
        return EV(plan.base, 1, dir, 2, plan.base_vals);
    }
    // the end of sweep it_: exchange between the bond groups, stopping rule and summary, quadrature -- in one of three forms
    int enqueue_sweep_end(int it_)
    {
        const int slot = it_ & 1;
        if (L.side) return end_side(it_);
        if (L.forkq) HIPCHECK(hipStreamWaitEvent(st, h->ev_val[slot ^ 1], 0));   // the previous quadrature is done with the boundaries
        if (int rc = L.tail ? end_tail(it_) : end_classic(it_)) return rc;
        if (L.pipe) HIPCHECK(hipEventRecord(h->ev_sum[slot], st));     // the summary of the sweep is in the pinned slot
        if (!P.has_quad) return TTX_OK;
        if (L.forkq) HIPCHECK(hipStreamWaitEvent(h->qstream, h->ev_sum[slot], 0));    // fork point = end of the sweep's main-stream work
        return enqueue_quadrature(it_, L.forkq ? h->qstream : st);
    }
    int tail_lean() const { return h->sel.tail_lean ? 1 : 0; }      // the form of the boundary blocks (ttx_exchange.h)
    // side: one launch on the main stream; the rest of the sweep's end goes to the quadrature's stream (enqueue_side)
    int end_side(int it_)
    {
        const int slot = it_ & 1;
        HIPCHECK(hipStreamWaitEvent(st, h->ev_val[slot ^ 1], 0));       // the previous quadrature is done with the boundaries and with rq
        KScope ks(h, TTX_K_EXCHANGE, 1);
        // ev_tail is the dispatch packet's own completion signal: no marker packet stands between the tail and the next sweep kernel
        if (h->sel.tail_event_kernel && !h->tail_event_retired) {
            const KLaunch &k = plan.exch_tail;
            int lean = tail_lean();
            void *args[] = {(void *)&P, (void *)&it_, (void *)&lean};
            if (hipExtLaunchKernel(k.fn, k.grid, k.block, args, k.lds, st, nullptr, h->ev_tail[slot], 0) == hipSuccess) return TTX_OK;
            (void)hipGetLastError();
            h->tail_event_retired = true; h->tail_event_fallbacks++;
        }
        launch(st, plan.exch_tail, P, it_, tail_lean());
        HIPCHECK(hipEventRecord(h->ev_tail[slot], st));
        return TTX_OK;
    }
    // tail: MAX / apply and the boundary blocks as independent blocks of one launch (the cluster kernel packed at its end), then the rule
    int end_tail(int it_)
    {
        { KScope ks(h, TTX_K_EXCHANGE, 1); launch(st, plan.exch_tail, P, it_, tail_lean()); }
        hipLaunchKernelGGL(k_sweep_end, dim3(1), dim3(256), 0, st, P, it_, h->h_sum_base + (size_t)(it_ & 1) * h->SB, 1);
        return TTX_OK;
    }
    // classic: the per-sweep exchange between bond groups (:763-961) launch by launch, then in the pipelined loop the rule: with one
    // process straight into the pinned slot, with several this GPU's part -> SUM all-reduce -> pinned slot, all stream-ordered
    int end_classic(int it_)
    {
        {
            KScope ks(h, TTX_K_EXCHANGE, (h->W > 1 ? 4 : 2) + (nproc > 1 ? 1 : 0));
            if (!cluster) hipLaunchKernelGGL(k_exch_pack, dim3(G), dim3(256), 0, st, P, 0);     // the cluster kernel packs at its end
            if (h->W > 1) {
                hipLaunchKernelGGL(k_exch_localmax, dim3(1), dim3(64), 0, st, P);
                if (int rc = xfer_neighbours(h)) return rc;
                if (int rc = allreduce_dev(h, P.redsend, P.redrecv, 4, 1)) return rc;
            }
            hipLaunchKernelGGL(k_exch_max_apply, dim3(G), dim3(256), lds_fpersist(P), st, P, h->W > 1 ? 1 : 0, nproc > 1 ? 1 : 0);
            if (nproc > 1) { if (int rc = EV(plan.exch_boundary, tail_lean())) return rc; }
        }
        double *const pinned = h->h_sum_base + (size_t)(it_ & 1) * h->SB;
        if (L.pipe) hipLaunchKernelGGL(k_sweep_end, dim3(1), dim3(256), 0, st, P, it_, h->W > 1 ? P.sumsend : pinned, 0);
        if (L.pipe && h->W > 1) {
            if (int rc = allreduce_dev(h, P.sumsend, P.sumrecv, h->SB, 0)) return rc;
            HIPCHECK(hipMemcpyAsync(pinned, P.sumrecv, sizeof(double) * h->SB, hipMemcpyDeviceToHost, st));
        }
        return TTX_OK;
    }
    // the per-sweep quadrature on the stream sq; in the pipelined loop its value goes to the pinned slot, ev_val behind it
    int enqueue_quadrature(int it_, hipStream_t sq)
    {
        const int slot = it_ & 1;
        KScope ks(h, TTX_K_QUAD, nproc > 1 ? 3 : 2);
        if (int rc = launch_quad(h, sq, L.pipe ? Pq : P, 0, P.quadw, L.fin_early ? h->ev_qb[slot] : nullptr)) return rc;
        if (L.pipe) {
            HIPCHECK(hipMemcpyAsync(h->h_val + slot, &P.gs[0].val, sizeof(double), hipMemcpyDeviceToHost, sq));
            HIPCHECK(hipEventRecord(h->ev_val[slot], sq));
        }
        return h->cb_error ? fail(TTX_EHIP, "host transport: a sendrecv / allreduce callback failed") : TTX_OK;
    }
    // side: what the end of sweep it_ leaves to the quadrature's stream behind the tail launch (ev_tail): the summary, the quadrature
    int enqueue_side(int it_)
    {
        const int slot = it_ & 1;
        hipStream_t sq = h->qstream;
        HIPCHECK(hipStreamWaitEvent(sq, h->ev_tail[slot], 0));
        hipLaunchKernelGGL(k_sweep_summary, dim3(1), dim3(256), 0, sq, P, it_, h->h_sum_base + (size_t)slot * h->SB);
        HIPCHECK(hipEventRecord(h->ev_sum[slot], sq));          // the summary of the sweep is in the pinned slot
        return enqueue_quadrature(it_, sq);
    }
    // finalise (:1029): dtt_lua shifts the rightmost inv of every group to its neighbour first (LoopPlan::final_exchange).  Enqueued
    // once (LoopPlan::pipe); after_val >= 0: the slot whose forked quadrature still reads the cores the finalisation overwrites.
    // With LoopPlan::fin_early that wait is for the quadrature's k_quad_build only.  The clearing of ctl[0..2], the final k_collect and
    // its copy (into the other pinned slot) are enqueued at once on the QUADRATURE's stream: there they stand behind k_quad_tree, which
    // reads ctl[2], and behind the value's copy by stream order, with no hop between two streams at the very end (a hop costs 11-12 us
    // here).  The one thing of the main stream they must follow is the speculative sweep kernel, which may read ctl[0]: an event
    // recorded behind it, in front of the main stream's own wait, has long fired by then.  They do not wait for the LU kernels or a
    // final exchange: k_collect reads the own bonds' ranks, the tapes and the groups' counters, none of which those write.
    // The run ends when both streams have: readback_wait and ev_fin.
    int enqueue_final(int after_val)
    {
        if (fin_enqueued) return TTX_OK;
        fin_enqueued = true;
        const bool early = L.fin_early && after_val >= 0;
        if (early) HIPCHECK(hipEventRecord(h->ev_fin[0], st));      // behind the speculative sweep kernel, in front of the wait below
        if (after_val >= 0) HIPCHECK(hipStreamWaitEvent(st, early ? h->ev_qb[after_val] : h->ev_val[after_val], 0));
        if (!early) HIPCHECK(hipMemsetAsync(P.ctl, 0, sizeof(int) * 3, st));      // ctl[3] (fault counter of the team / relay half-steps) is read by ttx_run afterwards
        {
            KScope ks(h, TTX_K_OTHER, 2);
            if (L.final_exchange(sweeps)) {
                hipLaunchKernelGGL(k_exch_pack, dim3(G), dim3(256), 0, st, P, 1);
                if (int rc = xfer_neighbours(h)) return rc;
                hipLaunchKernelGGL(k_exch_apply, dim3(G), dim3(256), lds_fpersist(P), st, P);
            }
            launch(st, plan.fin_luar, P, plan.fl);
            launch(st, plan.fin_lual, P, plan.fl);
        }
        if (!early) return TTX_OK;
        const hipStream_t sq = h->qstream;
        HIPCHECK(hipStreamWaitEvent(sq, h->ev_fin[0], 0));
        HIPCHECK(hipMemsetAsync(P.ctl, 0, sizeof(int) * 3, sq));
        sum_final = h->h_sum_base + (size_t)(after_val ^ 1) * h->SB;   // the finished sweep's slot is still to be read by process_sweep
        if (int rc = readback_enqueue(h, sum_final, sq)) return rc;
        HIPCHECK(hipEventRecord(h->ev_fin[1], sq));
        return TTX_OK;
    }
    // the record and the log line of sweep it_ (0: the initial cross) from the summary in h_sum and from val
    void record(int it_, int dir)
    {
        ttx_sweep_rec r{};
        r.it = it_; r.dir = dir; r.erank = erank_host(h, rank0_view(h, it_).data()); r.neval = (int64_t)h->h_sum[SUM_NEVAL]; r.val = val;
        r.amax = h->h_sum[SUM_AMAX]; r.pivotmax = it_ ? h->h_sum[SUM_PMAX] : -1; r.pivotmin = it_ ? h->h_sum[SUM_PMIN] : -1; r.seconds = since();
        h->recs.push_back(r);
        if (h->cfg.verbose) print_line(h, r, val_prev);
    }
    // host side of a finished sweep: stopping rule (identical to k_sweep_end), record, tapes, log line
    int process_sweep(int it_)
    {
        const int slot = it_ & 1;
        sweeps = it_;
        if (L.pipe) {
            HIPCHECK(hipEventSynchronize(h->ev_sum[slot]));
            h->h_sum = h->h_sum_base + (size_t)slot * h->SB;
        } else if (int rc = readback(h)) return rc;
        const StopRule sr = stop_rule(it_, h->cfg.maxrank, h->cfg.accuracy, h->h_sum[SUM_PMAX], h->h_sum[SUM_AMAX], strike);   // :1011-1019 (rank 0's amax, global pivotmax)
        // the rule needs only the summary: if it fires, the finalisation goes out before the host waits for the value
        if (L.pipe && sr.ready) if (int rc = enqueue_final(P.has_quad ? slot : -1)) return rc;
        if (P.has_quad) {
            if (L.pipe) { HIPCHECK(hipEventSynchronize(h->ev_val[slot])); val = h->h_val[slot]; }
            else val = h->h_sum[SUM_VAL];      // every GPU ran the same tree on the same gathered matrices
        }
        HIPCHECK(hipGetLastError());
        if (cluster && *(volatile int *)h->h_abort) { h->cluster_aborted = true; return fail(TTX_EHIP, "cluster sweep kernel: barrier timed out (workgroups of a bond group were not co-resident)"); }
        record(it_, 2 - it_ % 2);
        const size_t o = h->tapes.size();
        h->tapes.resize(o + (size_t)(d + 1) * 4, -1);
        for (int p = 1; p < d; p++) for (int x = 0; x < 4; x++) h->tapes[o + (size_t)p * 4 + x] = (int32_t)sum_bond(h, p)[1 + x];
        val_prev = val;
        strike = sr.strikes;
        ready = ready || sr.ready;
        return TTX_OK;
    }
    // preparation, the main loop (:309-1020) host-synchronised or pipelined, finalisation
    int run()
    {
        if (int rc = prepare()) return rc;
        if (!L.pipe) {
            for (int it = 1; !ready; it++) {
                if (int rc = (cluster || fused) ? launch_sweep_kernel(it) : enqueue_chain_sweep(it)) return rc;
                if (int rc = enqueue_sweep_end(it)) return rc;
                if (int rc = process_sweep(it)) return rc;
            }
        } else if (!ready) {
            if (L.forkq) { HIPCHECK(hipEventRecord(h->ev_val[0], h->qstream)); HIPCHECK(hipEventRecord(h->ev_val[1], h->qstream)); }
            if (!L.head) if (int rc = launch_sweep_kernel(1)) return rc;
            for (int it = 1; !ready; it++) {
                if (int rc = enqueue_sweep_end(it)) return rc;
                if (it + 1 < h->cfg.maxrank) if (int rc = launch_sweep_kernel(it + 1)) return rc;
                if (L.side) if (int rc = enqueue_side(it)) return rc;
                if (int rc = process_sweep(it)) return rc;
            }
        }
        if (int rc = enqueue_final(-1)) return rc;
        if (sum_final) h->h_sum = sum_final;
        if (int rc = sum_final ? readback_wait(h) : readback(h)) return rc;
        if (sum_final) HIPCHECK(hipEventSynchronize(h->ev_fin[1]));
        HIPCHECK(hipGetLastError());
#ifdef TTX_STAMPS
        if (int rc = dump_stamps(h)) return rc;
#endif
        h->neval = (int64_t)h->h_sum[SUM_NEVAL];
        h->k_bytes[TTX_K_HALFSTEP] += h->h_sum[SUM_BYTES];
        h->n_resid = (int64_t)h->h_sum[SUM_NRESID];
        h->rfinal = global_ranks(h);
        h->seconds = since();
        h->ran = true;
        return TTX_OK;
    }
};
template <int FUN>
static int run_impl(ttx_engine *h) { return SweepRun<FUN>(h).run(); }

// f(std::integral_constant<int, FUN>) for the instantiation an engine's integrand runs with: the host's `fun`, the COS coefficients
// and a loaded device integrand share the two-pass kernels of FUN_HOST (slot_eval tells them apart).  `who` names the caller
// where the integrand has not been set yet.
template <class F>
static int with_fun(const ttx_engine *h, const char *who, F f)
{
    switch (h->cfg.fun_id) {
        case TTX_FUN_ISING: return f(std::integral_constant<int, FUN_ISING>());
        case TTX_FUN_STDNORM: return f(std::integral_constant<int, FUN_STDNORM>());
        case TTX_FUN_HOST:
            if (who && !h->hfun) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_host first", who);
            return f(std::integral_constant<int, FUN_HOST>());
        case TTX_FUN_COSCOEFF: return f(std::integral_constant<int, FUN_HOST>());
        case TTX_FUN_DEVICE:
            if (who && !h->dfun) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_device first", who);
            return f(std::integral_constant<int, FUN_HOST>());
        case TTX_FUN_TRAINS:
            if (who && !h->tfun) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_trains first", who);
            return f(std::integral_constant<int, FUN_HOST>());
        case TTX_FUN_PULLBACK:
            if (who && !(h->pfun && h->pfun->comb)) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_pullback with a combiner first", who);
            return f(std::integral_constant<int, FUN_HOST>());
        default: return f(std::integral_constant<int, FUN_MVN>());
    }
}

static void reset_kernel_stats(ttx_engine *h)
{
    for (int k = 0; k < TTX_K_NKINDS; k++) { h->k_launches[k] = 0; h->k_ms[k] = 0; h->k_bytes[k] = 0; }
}
static void drain(ttx_engine *h) { (void)hipStreamSynchronize(h->stream); (void)hipStreamSynchronize(h->qstream); }
// ctl[3] after a run: what the team and relay half-steps counted (cleared by k_reset at the start of a run only; the finalisation
// leaves it alone)
static int read_fault_counter(ttx_engine *h)
{
    int faults = 0;
    drain(h);
    if (hipMemcpy(&faults, h->P.ctl + 3, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) faults = 0;
    return faults;
}
// Nothing of the run behind is kept, whatever it returned: drain both streams (kernels behind an aborted one see ctl[0] and do
// nothing), clear the sticky error, retire what failed for this engine and run again -- all implementations give identical results.
static int replay(ttx_engine *h, void (*retire)(ttx_engine *))
{
    drain(h);
    (void)hipGetLastError();
    retire(h);
    reset_kernel_stats(h);
    return run_impl<FUN_ISING>(h);
}

extern "C" int ttx_run(ttx_engine *h)
{
    if (!h) return fail(TTX_EINVAL, "ttx_run: null handle");
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (h->cfg.fun_id == 0) return fail(TTX_ESTATE, "ttx_run: this engine holds a loaded tensor train and has no integrand");
    reset_kernel_stats(h);
    if (h->cfg.fun_id == TTX_FUN_TRAINS) {
        // the operands' blocks as they stand now, then the sweep of a device integrand; the figures of ttx_trainfun_last at the end
        if (int rc = tf_prepare(h, "ttx_run", true)) return rc;
        if (int rc = run_impl<FUN_HOST>(h)) return rc;
        return tf_finish(h);
    }
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) {
        // the layers' heads and blocks as they stand now, then the sweep of a device integrand; the figures of ttx_pullback_last at the end
        if (int rc = pb_prepare(h, "ttx_run", true, true)) return rc;
        if (int rc = run_impl<FUN_HOST>(h)) return rc;
        return pb_finish(h);
    }
    if (h->cfg.fun_id != TTX_FUN_ISING)
        return with_fun(h, "ttx_run", [&](auto fun) { h->host_calls = 0; return run_impl<decltype(fun)::value>(h); });
    h->cluster_aborted = false;
    int rc = run_impl<FUN_ISING>(h);
    // a wait inside the cluster kernel timed out: replay on the multi-kernel chain
    if (rc && h->cluster_aborted)
        rc = replay(h, [](ttx_engine *e) {
            *e->h_abort = 0;
            e->retired.cluster = true; e->cluster_aborted = false; e->cluster_fallbacks++;
            if (e->P.ising_id == 1) e->P.arith = 0;        // the closed form of Ising C lives in the cluster kernel only
        });
    // k_halfstep_det found more units than the grid the host sized from its bound on the ranks (never expected): replay without teams
    if (h->de_team() && !h->de_v5() && read_fault_counter(h)) {
        (void)hipGetLastError();
        if (h->W > 1) return fail(TTX_EHIP, "ttx_run: k_halfstep_det met a rank above the host's bound; set TTX_DE_TEAM=0");
        rc = replay(h, [](ttx_engine *e) { e->retired.de_team = true; e->det_fallbacks++; });
    }
    // the relay of k_halfstep_de5 reports a broken hand-over (bounded waits): replay with k_halfstep_de
    if (h->de_v5()) if (const int faults = read_fault_counter(h)) {
        (void)hipGetLastError();
        if (h->W > 1) return fail(TTX_EHIP, "ttx_run: the wave relay of k_halfstep_de5 broke (%d hand-overs); set TTX_DE_V5=0", faults);
        rc = replay(h, [](ttx_engine *e) { e->retired.de_v5 = true; e->de5_fallbacks++; });
    }
    return rc;
}

// one line per stage of the sweep an engine would run now (the chain path's lines also where a whole-sweep kernel is in use: they
// are what a fallback runs); usable right after ttx_create
extern "C" int ttx_plan_describe(const ttx_engine *h, char *buf, int64_t cap)
{
    if (!h || !buf || cap < 1) return fail(TTX_EINVAL, "ttx_plan_describe: null argument");
    if (h->cfg.fun_id == 0) return fail(TTX_ESTATE, "ttx_plan_describe: this engine holds a loaded tensor train and has no integrand");
    return with_fun(h, nullptr, [&](auto fun) {
        const ChainPlan p = chain_plan<decltype(fun)::value>(h);
        std::string s = std::string("path: ") + (h->cluster_nb() ? "cluster" : h->sel.fused ? "fused" : "chain") + "\ntables: " + p.tables.name + "\nlottery: ";
        if (h->cfg.pivoting < 0) s += "-";
        else s += p.lot_eval ? std::string(p.lottery.name) + " + " + p.lot_eval.name + " + " + p.lottery.name : std::string(p.lottery.name);
        s += "\nhalfstep: ";
        for (int t = 0; t < p.ntier; t++) s += std::string(t ? ", " : "") + p.half[t].k.name + (t + 1 < p.ntier ? "[<=" + std::to_string(p.half[t].upto) + "]" : "");
        if (h->cfg.pivoting < 0) s += std::string("\nfullpiv: ") + (p.fullpiv == ChainPlan::FP_MFMA ? "mfma" : p.fullpiv == ChainPlan::FP_COLUMNS ? "columns" : "plain");
        s += "\n";
        if ((int64_t)s.size() + 1 > cap) return fail(TTX_EINVAL, "ttx_plan_describe: the text needs %zu bytes", s.size() + 1);
        memcpy(buf, s.c_str(), s.size() + 1);
        return (int)TTX_OK;
    });
}

extern "C" int ttx_num_sweeps(const ttx_engine *h) { return h ? (int)h->recs.size() : 0; }
extern "C" int ttx_get_sweeps(const ttx_engine *h, ttx_sweep_rec *out, int cap)
{
    if (!h || !out) return fail(TTX_EINVAL, "ttx_get_sweeps: null argument");
    int n = std::min(cap, (int)h->recs.size());
    memcpy(out, h->recs.data(), sizeof(ttx_sweep_rec) * n);
    return TTX_OK;
}
extern "C" int ttx_get_tapes(const ttx_engine *h, int32_t *out, int64_t cap)
{
    if (!h || !out) return fail(TTX_EINVAL, "ttx_get_tapes: null argument");
    int64_t n = std::min<int64_t>(cap, (int64_t)h->tapes.size());
    memcpy(out, h->tapes.data(), sizeof(int32_t) * n);
    return TTX_OK;
}
extern "C" int64_t ttx_neval(const ttx_engine *h) { return h ? h->neval : 0; }
extern "C" double ttx_seconds(const ttx_engine *h) { return h ? h->seconds : 0.0; }
extern "C" int ttx_get_ranks(const ttx_engine *h, int32_t *r)
{
    if (!h || !r || !h->ran) return fail(TTX_ESTATE, "ttx_get_ranks: run first");
    memcpy(r, h->rfinal.data(), sizeof(int32_t) * (h->d + 1));
    return TTX_OK;
}
static int owner_of_core(const ttx_engine *h, int k)
{
    for (int g = 0; g < h->G; g++) {
        int first = h->own[h->g0 + g], last = h->own[h->g0 + g + 1] - 1;
        bool lastg = (h->g0 + g == h->cfg.nproc - 1);
        if (k >= first && (k <= last || (lastg && k == h->d))) return g;
    }
    return -1;
}
static double *core_dev(const ttx_engine *h, int k)
{
    const int g = owner_of_core(h, k), first = h->own[h->g0 + g];
    return h->P.arg + ((size_t)g * h->NC + (k - first)) * h->P.CS;
}
static void push_ranks(ttx_engine *h)
{
    std::vector<int32_t> rr((size_t)h->G * (h->d + 2), 1);
    for (int g = 0; g < h->G; g++) for (int p = 0; p <= h->d; p++) rr[(size_t)g * (h->d + 2) + p] = h->rfinal[p];
    (void)hipMemcpyAsync(h->P.r, rr.data(), sizeof(int32_t) * rr.size(), hipMemcpyHostToDevice, h->stream);
    (void)hipStreamSynchronize(h->stream);
}
// all-reduce (sum) of a device buffer of any length over the processes of the job, in place: the host transports stage through a
// pinned slot of red_cap doubles, so the buffer goes in pieces
static int allreduce_big(ttx_engine *h, double *buf, size_t count)
{
    if (h->W == 1) return TTX_OK;
    const size_t piece = h->comm ? count : std::max<size_t>(1, h->red_cap);
    int inflight = 0;
    for (size_t o = 0; o < count; o += piece) {
        if (int rc = allreduce_dev(h, buf + o, buf + o, std::min(piece, count - o), 0)) return rc;
        // host transports: a reduction's descriptor and pinned slot are recycled after NRED enqueues -- drain before that
        if (!h->comm && ++inflight >= ttx_engine::NRED - 2) { HIPCHECK(hipStreamSynchronize(h->stream)); inflight = 0; }
    }
    return TTX_OK;
}
static std::vector<int32_t> modes_of(const ttx_engine *h) { return std::vector<int32_t>(h->n1.begin() + 1, h->n1.begin() + 1 + h->d); }
// destroy an engine that an operation made and then failed on: the operation's error text stays the last error
// The finalised train of a MULTI-PROCESS job on every process, as a new single-process engine with the same integrand (`out`):
// each process copies the cores it holds into its slots of the new engine's core array and a SUM all-reduce over the job's transport
// fills in the others (their slots hold -0.0 here, the neutral element of fp addition for every value).  dtt_accchk, norm, dot_product, ort, svd and dtt_write of the
// reference work on a `type(dtt)` that holds ALL cores (lib/tt.f90, lib/dmrgg.f90:1081-1166): on a multi-process engine they go
// through this copy.  Collective: every process of the job must call it.
extern "C" int ttx_replicate(ttx_engine *h, ttx_engine **out)
{
    if (!h || !out) return fail(TTX_EINVAL, "ttx_replicate: null argument");
    *out = nullptr;
    if (!h->ran) return fail(TTX_ESTATE, "ttx_replicate: run dtt_dmrgg first");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const int d = h->d;
    ttx_config c = h->cfg;
    const std::vector<int32_t> nn = modes_of(h);
    std::vector<double> qw;
    c.n = nn.data(); c.par = h->par.empty() ? nullptr : h->par.data(); c.aux = h->aux.empty() ? nullptr : h->aux.data(); c.naux = (int32_t)h->aux.size();
    c.quadw = nullptr;
    if (!h->quadw.empty()) { for (int k = 1; k <= d; k++) for (int j = 0; j < h->n1[k]; j++) qw.push_back(h->quadw[(size_t)k * h->NM + j]); c.quadw = qw.data(); }
    c.nproc = 1; c.mybonds = nullptr; c.world_rank = 0; c.world_size = 1; c.verbose = 0; c.arith = h->arith();
    ttx_engine *e = nullptr;
    int rc = create_impl(&e, &c, h->cfg.fun_id == 0);
    if (rc) return rc;
    e->hfun = h->hfun; e->hfun_par = h->hfun_par;
    e->dfun = h->dfun;                              // same process, same device: the replica shares the module and the par copy
    e->tfun = h->tfun;                              // ... and the operand list of TTX_FUN_TRAINS
    e->pfun = h->pfun;                              // ... and the layers, reference grid and combiner of TTX_FUN_PULLBACK
    if (e->RM != h->RM || e->NM != h->NM) { ttx_destroy(e); return fail(TTX_EHIP, "ttx_replicate: layout mismatch"); }
    const size_t CS = h->P.CS;
    // slots of the other processes' cores hold -0.0: x + (-0.0) = x for EVERY x, also for x = -0.0 (x + (+0.0) would turn it into +0.0)
    hipLaunchKernelGGL(k_fill_const, dim3(1024), dim3(256), 0, h->stream, (size_t)d * CS, e->P.arg, -0.0);
    for (int k = 1; k <= d; k++) {
        if (owner_of_core(h, k) < 0) continue;
        HIPCHECK(hipMemcpyAsync(e->P.arg + (size_t)(k - 1) * CS, core_dev(h, k), sizeof(double) * CS, hipMemcpyDeviceToDevice, h->stream));
    }
    if ((rc = allreduce_big(h, e->P.arg, (size_t)d * CS))) { ttx_destroy(e); return rc; }
    // the run-time RNG stream continues where rank 0 of the reference left it (dtt_accchk draws from it): the position of the job's
    // FIRST bond group, handed to every process through the same kind of all-reduce (an integer below 2^53 is exact in a double)
    unsigned long long rp = 0;
    HIPCHECK(hipMemcpyAsync(&rp, &h->P.gs[0].rngpos, sizeof(rp), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if (h->W > 1) {
        double v = (h->g0 == 0) ? (double)rp : -0.0;
        double *dv = e->P.redsend;                      // a few doubles of the replica, not in use yet
        HIPCHECK(hipMemcpyAsync(dv, &v, sizeof(double), hipMemcpyHostToDevice, h->stream));
        if ((rc = allreduce_dev(h, dv, dv, 1, 0))) { ttx_destroy(e); return rc; }
        HIPCHECK(hipMemcpyAsync(&v, dv, sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        rp = (unsigned long long)v;
    }
    if (h->cb_error) { ttx_destroy(e); return fail(TTX_EHIP, "host transport: a sendrecv / allreduce callback failed"); }
    HIPCHECK(hipMemcpy(&e->P.gs[0].rngpos, &rp, sizeof(rp), hipMemcpyHostToDevice));
    e->rfinal = h->rfinal; e->neval = h->neval; e->ran = true;
    push_ranks(e);
    *out = e;
    return TTX_OK;
}
// run `fn` on a replica of a multi-process engine's train
template <class FN>
static int with_replica(ttx_engine *h, FN fn)
{
    ttx_engine *e = nullptr;
    int rc = ttx_replicate(h, &e);
    if (rc) return rc;
    rc = fn(e);
    if (rc) destroy_keep_error(e); else ttx_destroy(e);
    return rc;
}

extern "C" int64_t ttx_core_size(const ttx_engine *h, int k)
{
    if (!h || !h->ran || k < 1 || k > h->d || owner_of_core(h, k) < 0) return 0;
    return (int64_t)h->rfinal[k - 1] * h->n1[k] * h->rfinal[k];
}
extern "C" int ttx_get_core(const ttx_engine *h, int k, double *buf)
{
    if (!h || !buf || !h->ran) return fail(TTX_ESTATE, "ttx_get_core: run first");
    if (k < 1 || k > h->d) return fail(TTX_EINVAL, "ttx_get_core: core %d out of range", k);
    int g = owner_of_core(h, k);
    if (g < 0) return fail(TTX_EINVAL, "ttx_get_core: core %d is not held by this process", k);
    const int r0 = h->rfinal[k - 1], r1 = h->rfinal[k], n = h->n1[k], first = h->own[h->g0 + g];
    const double *src = h->P.arg + ((size_t)g * h->NC + (k - first)) * h->P.CS;
    // strided device -> compact host: one 2D copy per right-rank slab (pure data movement)
    for (int s = 0; s < r1; s++)
        HIPCHECK(hipMemcpy2D(buf + (size_t)r0 * n * s, sizeof(double) * r0, src + h->P.SS * s, sizeof(double) * h->RM, sizeof(double) * r0, n, hipMemcpyDeviceToHost));
    return TTX_OK;
}

// ---- tensor trains from outside the sweep: host cores and the reference's stream file ----------------
extern "C" int ttx_get_modes(const ttx_engine *h, int32_t *d, int32_t *n)
{
    if (!h || !d) return fail(TTX_EINVAL, "ttx_get_modes: null argument");
    *d = h->d;
    if (n) for (int k = 1; k <= h->d; k++) n[k - 1] = h->n1[k];
    return TTX_OK;
}

// a new single-process engine without integrand whose resident train has the given modes and ranks; the cores are the caller's to fill
static int train_shell(ttx_engine **out, const char *who, int32_t d, const int32_t *n, const int32_t *r, int32_t device)
{
    *out = nullptr;
    if (d < 2) return fail(TTX_EINVAL, "%s: at least two cores are needed (got %d)", who, d);
    int rmax = 1;
    for (int k = 0; k <= d; k++) { if (r[k] < 1) return fail(TTX_EINVAL, "%s: rank r(%d)=%d", who, k, r[k]); rmax = std::max(rmax, (int)r[k]); }
    // ort/svd may pass through r(k) = min(r(k-1)*n(k), ...) <= the incoming ranks, so max(r) is enough storage
    ttx_config c{};
    c.d = d; c.n = n; c.fun_id = 0; c.accuracy = -1.0; c.maxrank = rmax; c.pivoting = 0; c.nproc = 1; c.device = device; c.world_size = 1;
    ttx_engine *h = nullptr;
    int rc = create_impl(&h, &c, true);
    if (rc) return rc;
    auto to_dev = [&](void *dst, const void *src, size_t bytes) {
        const hipError_t e = hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? TTX_OK : fail(TTX_EHIP, "%s: %s", who, hipGetErrorString(e));
    };
    GroupState g0{};                    // only the bond range is read by the quad kernels
    g0.first = 1; g0.last = d - 1; g0.gglobal = 0;
    std::vector<int32_t> rr((size_t)(d + 2), 1);
    for (int p = 0; p <= d; p++) rr[p] = r[p];
    if (!(rc = to_dev(h->P.gs, &g0, offsetof(GroupState, S)))) rc = to_dev(h->P.r, rr.data(), sizeof(int32_t) * rr.size());
    if (rc) { destroy_keep_error(h); return rc; }
    h->rfinal.assign(r, r + d + 1);
    h->ran = true;
    *out = h;
    return TTX_OK;
}
// a new train out of an operation: the shell, then fill(e) writes its cores; a fill that fails takes the shell with it and its error
// text stays, a fill that succeeds hands the engine to *out
template <class FN>
static int new_train(ttx_engine **out, const char *who, int32_t d, const int32_t *n, const int32_t *r, int32_t device, FN fill)
{
    *out = nullptr;
    ttx_engine *e = nullptr;
    int rc = train_shell(&e, who, d, n, r, device);
    if (rc) return rc;
    if ((rc = fill(e))) { destroy_keep_error(e); return rc; }
    *out = e;
    return TTX_OK;
}

extern "C" int ttx_from_tt(ttx_engine **out, int32_t d, const int32_t *n, const int32_t *r, const double *cores, int32_t device)
{
    if (!out || !n || !r || !cores) return fail(TTX_EINVAL, "ttx_from_tt: null argument");
    return new_train(out, "ttx_from_tt", d, n, r, device, [&](ttx_engine *h) {
        size_t off = 0;
        for (int k = 1; k <= d; k++) {
            const int r0 = r[k - 1], r1 = r[k], nk = n[k - 1];
            double *dst = h->P.arg + (size_t)(k - 1) * h->P.CS;
            for (int s = 0; s < r1; s++) {        // compact host -> padded device slabs (inverse of ttx_get_core)
                hipError_t e = hipMemcpy2D(dst + h->P.SS * s, sizeof(double) * h->RM, cores + off + (size_t)r0 * nk * s, sizeof(double) * r0, sizeof(double) * r0, nk, hipMemcpyHostToDevice);
                if (e != hipSuccess) return fail(TTX_EHIP, "ttx_from_tt: %s", hipGetErrorString(e));
            }
            off += (size_t)r0 * nk * r1;
        }
        return (int)TTX_OK;
    });
}

// the resident train of a single-process engine on the host, as the writers of ttx_files.h take it: the cores one after the other
static int train_to_host(const ttx_engine *h, std::vector<double> &x)
{
    size_t sz = 0, off = 0;
    for (int k = 1; k <= h->d; k++) sz += (size_t)ttx_core_size(h, k);
    x.resize(sz);
    for (int k = 1; k <= h->d; k++) { int rc = ttx_get_core(h, k, x.data() + off); if (rc) return rc; off += (size_t)ttx_core_size(h, k); }
    return TTX_OK;
}
extern "C" int ttx_write(const ttx_engine *h, const char *path)
{
    if (!h || !path || !h->ran) return fail(TTX_ESTATE, "dtt_write: no tensor train to write");
    if (h->W > 1) {     // collective: every process takes part in the replica, rank 0 writes the file
        ttx_engine *hh = const_cast<ttx_engine *>(h);
        return with_replica(hh, [&](ttx_engine *e) { return hh->wrank == 0 ? ttx_write(e, path) : TTX_OK; });
    }
    std::vector<double> x;
    std::string text;
    if (int rc = train_to_host(h, x)) return rc;
    if (int rc = ttfile_write(path, h->d, &h->n1[1], h->rfinal.data(), x.data(), &text)) return fail(rc, "%s", text.c_str());
    return TTX_OK;
}
extern "C" int ttx_write_hdf5(const ttx_engine *h, const char *path)
{
    if (!h || !path || !h->ran) return fail(TTX_ESTATE, "save_dtt_to_hdf5: no tensor train to write");
    if (h->W > 1) return fail(TTX_EINVAL, "save_dtt_to_hdf5: single-process engines only");
    std::vector<double> x;
    std::string text;
    if (int rc = train_to_host(h, x)) return rc;
    if (int rc = hdf5_write_tt(path, h->d, &h->n1[1], h->rfinal.data(), x.data(), &text)) return fail(rc, "%s", text.c_str());
    return TTX_OK;
}
extern "C" int ttx_read_hdf5(ttx_engine **out, const char *path, int32_t device)
{
    if (!out || !path) return fail(TTX_EINVAL, "ttx_read_hdf5: null argument");
    *out = nullptr;
    std::vector<int32_t> n, r;
    std::vector<double> cores;
    std::string text;
    if (int rc = hdf5_read_tt(path, n, r, cores, &text)) return fail(rc, "%s", text.c_str());
    return ttx_from_tt(out, (int32_t)n.size(), n.data(), r.data(), cores.data(), device);
}

extern "C" int ttx_read(ttx_engine **out, const char *path, int32_t device)
{
    if (!out || !path) return fail(TTX_EINVAL, "dtt_read: null argument");
    *out = nullptr;
    std::vector<int32_t> n, r;
    std::vector<double> x;
    std::string text;
    if (int rc = ttfile_read(path, n, r, x, &text)) return fail(rc, "%s", text.c_str());
    return ttx_from_tt(out, (int32_t)n.size(), n.data(), r.data(), x.data(), device);
}

// per-call device temporaries: released on every path out of the function that holds the guard
struct DevTmp {
    std::vector<void *> p;
    ~DevTmp() { for (void *q : p) (void)hipFree(q); }
    template <class T> hipError_t alloc(T **q, size_t count)
    {
        hipError_t e = hipMalloc((void **)q, sizeof(T) * count);
        if (e == hipSuccess) p.push_back((void *)*q);
        return e;
    }
};

extern "C" int ttx_quad(ttx_engine *h, const double *w, double *val)
{
    if (!h || !val || !h->ran) return fail(TTX_ESTATE, "ttx_quad: run first");
    HIPCHECK(hipSetDevice(h->cfg.device));
    DevTmp tmp;
    double *dw = nullptr;
    if (w) {
        std::vector<double> wp((size_t)(h->d + 1) * h->NM, 0.0);
        size_t off = 0;
        for (int k = 1; k <= h->d; k++) { for (int j = 0; j < h->n1[k]; j++) wp[(size_t)k * h->NM + j] = w[off + j]; off += h->n1[k]; }
        HIPCHECK(tmp.alloc(&dw, wp.size()));
        HIPCHECK(hipMemcpy(dw, wp.data(), sizeof(double) * wp.size(), hipMemcpyHostToDevice));
    }
    int rc = launch_quad(h, h->stream, h->P, 1, dw);
    if (!rc) rc = readback(h);
    if (rc) return rc;
    HIPCHECK(hipGetLastError());
    *val = h->h_sum[SUM_VAL];
    return TTX_OK;
}

template <int FUN>
static int accchk_impl(ttx_engine *h, int nlot, double *einf, double *efro, double *ainf, double *afro, int32_t *pivot)
{
    DevProb &P = h->P;
    const int d = h->d;
    std::vector<int> owner(d + 2, 0);
    for (int k = 1; k <= d; k++) owner[k] = owner_of_core(h, k);
    // the stream position where dtt_dmrgg left the run-time generator (rank 0 of the reference = group 0)
    GroupState g0s;
    HIPCHECK(hipMemcpy(&g0s, P.gs, sizeof(GroupState), hipMemcpyDeviceToHost));
    DevTmp tmp;
    int *downer, *dind; double *dout;
    HIPCHECK(tmp.alloc(&downer, d + 2)); HIPCHECK(tmp.alloc(&dind, (size_t)nlot * d)); HIPCHECK(tmp.alloc(&dout, 4 * (size_t)nlot));
    HIPCHECK(hipMemcpy(downer, owner.data(), sizeof(int) * (d + 2), hipMemcpyHostToDevice));
    const size_t lds = sizeof(double) * (h->par.size() + 2 * h->RM + 4) + sizeof(int) * (d + 4);
    auto check = [&](const DevProb &Q, int count, int il0) {
        hipLaunchKernelGGL(k_accchk<FUN>, dim3(count), dim3(64), lds, h->stream, Q, (unsigned long long)g0s.rngpos, nlot, (const int *)downer, dout, dind, il0);
    };
    if (FUN == FUN_HOST) {
        // chunks of at most G*HS samples: index pass, the user's function on the host, value pass
        const int chunk = (int)std::min<size_t>((size_t)h->G * h->sel.HS, 65535);
        for (int il0 = 0; il0 < nlot; il0 += chunk) {
            const int cnt = std::min(chunk, nlot - il0);
            DevProb Q = P;
            Q.hostpass = 1;
            check(Q, cnt, il0);
            if (int rc_ = slot_eval(h)) return rc_;
            Q.hostpass = 2;
            check(Q, cnt, il0);
        }
    } else
        check(P, nlot, 0);
    std::vector<double> o(4 * (size_t)nlot);
    std::vector<int> ind((size_t)nlot * d);
    HIPCHECK(hipMemcpyAsync(o.data(), dout, sizeof(double) * o.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(ind.data(), dind, sizeof(int) * ind.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    // the reference's sequential bookkeeping over the samples (:1126-1133): strict '<' keeps the first worst sample
    double e1 = 0.0, e2 = 0.0, a1 = 0.0, a2 = 0.0; int worst = -1;
    for (int il = 0; il < nlot; il++) {
        if (e1 < o[4 * (size_t)il]) { e1 = o[4 * (size_t)il]; worst = il; }
        e2 = e2 + o[4 * (size_t)il + 1];
        a1 = std::max(a1, o[4 * (size_t)il + 2]);
        a2 = a2 + o[4 * (size_t)il + 3];
    }
    *einf = e1; *efro = std::sqrt(e2); *ainf = a1; *afro = std::sqrt(a2);
    if (pivot && worst >= 0) for (int i = 0; i < d; i++) pivot[i] = ind[(size_t)worst * d + i];
    return TTX_OK;
}

extern "C" int ttx_accchk(ttx_engine *h, int32_t nlot, double *einf, double *efro, double *ainf, double *afro, int32_t *pivot)
{
    if (h && h->cfg.fun_id == TTX_FUN_TRAINS && !h->tfun) return fail(TTX_ESTATE, "ttx_accchk: call ttx_set_integrand_trains first");
    if (h && h->cfg.fun_id == TTX_FUN_PULLBACK && !(h->pfun && h->pfun->comb)) return fail(TTX_ESTATE, "ttx_accchk: call ttx_set_integrand_pullback with a combiner first");
    if (!h || !einf || !efro || !ainf || !afro || !h->ran) return fail(TTX_ESTATE, "ttx_accchk: run first");
    if (h->W > 1)       // every rank needs all cores: the check runs on a replica of the job's train (identical result on every process)
        return with_replica(h, [&](ttx_engine *e) { return ttx_accchk(e, nlot, einf, efro, ainf, afro, pivot); });
    if (nlot < 1) return fail(TTX_EINVAL, "dtt_accchk: nlot must be positive");
    if (h->cfg.fun_id == 0) return fail(TTX_ESTATE, "dtt_accchk: this engine holds a loaded tensor train and has no integrand");
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (h->cfg.fun_id == TTX_FUN_TRAINS) if (int rc = tf_prepare(h, "dtt_accchk", false)) return rc;
    if (h->cfg.fun_id == TTX_FUN_PULLBACK) if (int rc = pb_prepare(h, "dtt_accchk", false, true)) return rc;
    return with_fun(h, "dtt_accchk", [&](auto fun) { return accchk_impl<decltype(fun)::value>(h, nlot, einf, efro, ainf, afro, pivot); });
}

// ---- tt_lib utilities (ort / svd / norm / dot) -------------------------------------------------------------
// The factorisation scratch Sm (doubles) and Si (ints): five RM x RM matrices (three more are spare), then vectors and scalars
struct TtScratch {
    double *Rm, *Rt, *Vb, *US, *Vs;     // R of a QR, its transpose, V of the Jacobi SVD, the kept U S and V columns
    double *tau, *sv;                   // reflector scales, singular values (RM each)
    double *acc, *sums;                 // ort_impl: sum of log norms, last 1/norm; sumsq: sum of squares, exponent
    int *perm, *info;                   // Jacobi: order of the singular values; rank and sweeps
    static size_t doubles(size_t RM) { return 8 * RM * RM + 4 * RM + 16; }
    static size_t ints(size_t RM) { return 2 * RM + 16; }
    explicit TtScratch(const ttx_engine *h)
    {
        const size_t RM = h->RM, M = RM * RM;
        Rm = h->Sm; Rt = Rm + M; Vb = Rm + 2 * M; US = Rm + 3 * M; Vs = Rm + 4 * M;
        tau = Rm + 8 * M; sv = tau + RM; acc = tau + 4 * RM + 2; sums = tau + 4 * RM + 4;
        perm = h->Si; info = h->Si + RM;
    }
};
static int tt_prepare(ttx_engine *h, const char *who)
{
    if (!h || !h->ran) return fail(TTX_ESTATE, "%s: run dtt_dmrgg first", who);
    if (h->W > 1) return fail(TTX_EINVAL, "%s: single-process engines only", who);
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (!h->Wa) {
        const size_t CS = h->P.CS, RM = h->RM;
        int rc;
        if ((rc = dev_alloc(h, &h->Wa, CS)) || (rc = dev_alloc(h, &h->Wb, CS)) || (rc = dev_alloc(h, &h->Wc, CS)) || (rc = dev_alloc(h, &h->Wd, CS))) return rc;
        if ((rc = dev_alloc(h, &h->Sm, TtScratch::doubles(RM))) || (rc = dev_alloc(h, &h->Si, TtScratch::ints(RM)))) return rc;
    }
    return TTX_OK;
}
static inline dim3 g1(size_t n) { return dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)); }
// core k between its place in the train and a dense column-major r0 n x r1 matrix (trans: its transpose); e's current ranks
static size_t core_elems(const ttx_engine *e, int k) { return (size_t)e->rfinal[k - 1] * e->n1[k] * e->rfinal[k]; }
static void pack_core(hipStream_t st, const ttx_engine *e, int k, double *dst, int trans = 0)
{
    hipLaunchKernelGGL(k_pack_core, g1(core_elems(e, k)), dim3(256), 0, st, core_dev(e, k), dst, e->rfinal[k - 1], e->n1[k], e->rfinal[k], e->RM, e->P.SS, trans);
}
static void unpack_core(ttx_engine *h, int k, const double *src, int r0, int r1, int trans = 0)
{
    hipLaunchKernelGGL(k_unpack_core, g1((size_t)r0 * h->n1[k] * r1), dim3(256), 0, h->stream, core_dev(h, k), src, r0, h->n1[k], r1, h->RM, h->P.SS, trans, 1.0);
}
static void scal_core(ttx_engine *h, int k, double a)
{
    hipLaunchKernelGGL(k_scal_core, g1(core_elems(h, k)), dim3(256), 0, h->stream, core_dev(h, k), h->rfinal[k - 1], h->n1[k], h->rfinal[k], h->RM, h->P.SS, a);
}
// out (rows x rr) = the columns perm[0..rr) of X (rows x rows), each times sv[perm[j]] (if given) and sdiv
static void take_cols(ttx_engine *h, int rows, int rr, const double *X, const int *perm, const double *sv, double sdiv, double *out)
{
    hipLaunchKernelGGL(k_take_cols, g1((size_t)rows * rr), dim3(256), 0, h->stream, rows, rr, X, rows, perm, sv, sdiv, out);
}
// threads of the one-workgroup factorisation kernels (a multiple of 64, at most 1024): the kernels are chains of short phases
// separated by workgroup barriers, whose cost grows with the number of waves -- TTX_QR_THREADS / TTX_JAC_THREADS override
static int tt_threads(const char *env, int dflt) { return std::max(64, std::min(1024, env_int(env, dflt))) & ~63; }
static int gemm(ttx_engine *h, int M, int N, int K, const double *A, int lda, const double *B, int ldb, double *C, int ldc)
{
    hipLaunchKernelGGL(k_gemm_mfma, dim3((N + 63) / 64, (M + 15) / 16), dim3(256), 0, h->stream, M, N, K, A, lda, B, ldb, C, ldc);
    return TTX_OK;
}
// core k-1 times B (r[k-1] x rr): the new bond rank rr is the caller's to record (lib/tt.f90:344)
static void push_left(ttx_engine *h, int k, const double *B, int rr)
{
    const int mm = h->rfinal[k - 1], kk = h->rfinal[k - 2] * h->n1[k - 1];
    pack_core(h->stream, h, k - 1, h->Wb);
    gemm(h, kk, rr, mm, h->Wb, kk, B, mm, h->Wc, kk);
    unpack_core(h, k - 1, h->Wc, h->rfinal[k - 2], rr);
}
// B (mn x r[k]) times core k+1, and r[k] = mn (:175)
static void push_right(ttx_engine *h, int k, const double *B, int mn)
{
    const int nn = h->rfinal[k], kk = h->n1[k + 1] * h->rfinal[k + 1];
    pack_core(h->stream, h, k + 1, h->Wb);
    gemm(h, mn, kk, nn, B, mn, h->Wb, nn, h->Wc, mn);
    h->rfinal[k] = mn;
    unpack_core(h, k + 1, h->Wc, mn, h->rfinal[k + 1]);
}
// ---- QR of an unfolding: the plan of ttx_qr_plan.h, its LDS ceilings, its launches in order ------------------------------------
static const void *qr_kernel(const QrLaunch &L)
{
    if (L.kernel == QRK_OWN) {
#define QRO(MRv, NCv) if (L.mr == MRv && L.nc == NCv) return reinterpret_cast<const void *>(k_qr_own<MRv, NCv>);
        QRO(2, 1) QRO(4, 1) QRO(8, 1) QRO(2, 2) QRO(4, 2) QRO(8, 2) QRO(2, 4) QRO(4, 4) QRO(2, 8) QRO(4, 8)
#undef QRO
    }
    if (L.kernel == QRK_PANEL) return reinterpret_cast<const void *>(k_qr_panel);
    if (L.kernel == QRK_LDS) return reinterpret_cast<const void *>(k_qr<true>);
    if (L.kernel == QRK_STREAM) return reinterpret_cast<const void *>(k_qr<false>);
    return nullptr;
}
// one launch of the plan: M (rows x n, P panels of rbs rows) -> Q (M itself for a top launch), triangles to R (leading dimension ldr)
static int qr_launch(ttx_engine *h, const QrLaunch &L, int n, const double *M, double *Q, double *R, int ldr, int rstep, double *tau)
{
    const void *fn = qr_kernel(L);
    const bool agree = L.kernel == QRK_OWN ? L.lds == sizeof(double) * qr_own_lds_doubles(L.rbs, n) :
                       L.kernel == QRK_PANEL ? L.lds == sizeof(double) * qr_panel_lds_doubles(L.rbs, n) : true;
    if (!fn || !agree) return fail(TTX_EHIP, "qr: the plan of %d x %d names no kernel or disagrees with it on LDS", L.rows, n);
    int rows = L.rows, rbs = L.rbs;
    void *own[] = {&rows, &n, &rbs, &M, &rows, &Q, &rows, &R, &ldr, &rstep, &tau}, *panel[] = {&rows, &n, &rbs, &M, &Q, &R, &ldr}, *whole[] = {&rows, &n, &Q, &R, &tau};
    hipError_t e = hipLaunchKernel(fn, dim3(L.P), dim3(L.threads), L.kernel == QRK_OWN ? own : L.kernel == QRK_PANEL ? panel : whole, L.lds, h->stream);
    if (e != hipSuccess && L.kernel == QRK_OWN) return fail(TTX_EHIP, "k_qr_own: %s", hipGetErrorString(e));
    return TTX_OK;
}
// A (m x n) -> Q in place, R (min(m, n) x n).  The tall-skinny route keeps the Q panels of level 0 in Wb, the stacked triangles of
// the levels (then their accumulated Q) in Wc and the Q panels of the levels >= 1 in Wd -- all free while a qr() is running.
static int qr(ttx_engine *h, int m, int n, double *A, double *R, double *tau)
{
    QrEnv env;
    env.own_off = env_off("TTX_QR_OWN"); env.tsqr_off = env_off("TTX_TSQR"); env.panel = env_int("TTX_QR_PANEL", 0);
    env.threads = tt_threads("TTX_QR_THREADS", 1024); env.top_threads = tt_threads("TTX_QRTOP_THREADS", 1024);
    const QrPlan p = qr_plan(m, n, A == h->Wa, env);
    if (p.route == QR_REFUSED) return fail(TTX_EINVAL, "dtt_ort: unfolding with %d rows does not fit the LDS-staged reflector", m);
    int rc;
    for (const QrLevel &L : p.lv) if ((rc = ensure_lds(h, qr_kernel(L), L.lds))) return rc;
    if ((rc = ensure_lds(h, qr_kernel(p.top), p.top.lds))) return rc;
    for (size_t l = 0; l < p.lv.size(); l++) {                                  // a level's triangles are the next level's matrix (P n x n)
        const QrLevel &L = p.lv[l];
        if ((rc = qr_launch(h, L, n, l ? h->Wc + L.m_off : A, l ? h->Wd + L.q_off : h->Wb, h->Wc + L.r_off, L.P * n, n, nullptr))) return rc;
    }
    double *top = p.lv.empty() ? A : h->Wc + p.top_off;                         // one workgroup, in place: top -> Q_top (rows x n), R (n x n)
    if ((rc = qr_launch(h, p.top, n, top, top, R, std::min(p.top.rows, n), 0, tau))) return rc;
    // explicit Q, top down: Qacc(level l) = blockdiag(Q_p) * Qacc(level l+1); level l's own matrix buffer takes the result
    const double *Qup = top; int ldup = p.top.rows;
    for (int l = (int)p.lv.size() - 1; l >= 0; l--) {
        const QrLevel &L = p.lv[l];
        double *out = l ? h->Wc + L.m_off : A;
        hipLaunchKernelGGL(k_gemm_mfma_panels, dim3((n + 63) / 64, (L.rbs + 15) / 16, L.P), dim3(256), 0, h->stream,
                           L.rows, n, L.rbs, (const double *)(l ? h->Wd + L.q_off : h->Wb), L.rows, Qup, ldup, out, L.rows);
        Qup = out; ldup = L.rows;
    }
    return TTX_OK;
}
static int jacobi(ttx_engine *h, int p, int q, double *X, double *V, double *sv, int *perm, int *info, double tol, int rmax)
{
    const size_t lds = sizeof(double) * ((size_t)p + q) * q;
    const int in_lds = lds <= TTX_LDS_JACOBI;
    if (in_lds) { if (int rc = ensure_lds(h, reinterpret_cast<const void *>(k_jacobi_svd), lds)) return rc; }
    hipLaunchKernelGGL(k_jacobi_svd, dim3(1), dim3(tt_threads("TTX_JAC_THREADS", 256)), in_lds ? lds : 0, h->stream, p, q, X, V, sv, perm, info, 1, tol, rmax, in_lds);
    return TTX_OK;
}
// ||x||_2 = sqrt(*s2) 2^*e (e = 0 unless the plain sum of squares left [1e-280, 1e280], ttx_ttops.h)
static int sumsq(ttx_engine *h, size_t n, const double *x, double *s2, int *e)
{
    double *d = TtScratch(h).sums;
    double out[2];
    hipLaunchKernelGGL(k_sumsq, dim3(1), dim3(1024), 0, h->stream, n, x, d);
    HIPCHECK(hipMemcpyAsync(out, d, 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    *s2 = out[0]; *e = (int)out[1];
    return TTX_OK;
}
// sqrt(sum v[j]^2) on the host with the same rescaled second pass
static double host_norm(const double *v, int n)
{
    double s2 = 0.0;
    for (int j = 0; j < n; j++) s2 += v[j] * v[j];
    if (s2 > 1e-280 && s2 < 1e280) return std::sqrt(s2);
    double m = 0.0;
    for (int j = 0; j < n; j++) m = std::max(m, std::fabs(v[j]));
    if (m == 0.0 || !std::isfinite(m)) return std::sqrt(s2);
    int e; (void)std::frexp(m, &e);
    double p = 0.0;
    for (int j = 0; j < n; j++) { const double y = std::ldexp(v[j], -e); p += y * y; }
    return std::ldexp(std::sqrt(p), e);
}

static int ort_impl(ttx_engine *h)
{
    const int d = h->d;
    std::vector<int32_t> &r = h->rfinal;
    const TtScratch s(h);
    int rc;
    HIPCHECK(hipMemsetAsync(s.acc, 0, 2 * sizeof(double), h->stream));
    // the whole left-to-right pass is enqueued without a host round trip: the new ranks min(r0*n, r1) are known on the
    // host, the norm equalisation (log of each R's norm, final rescaling) stays on the device
    for (int k = 1; k <= d - 1; k++) {                                  // lib/tt.f90:149-181
        const int r0 = r[k - 1], mm = r0 * h->n1[k], nn = r[k], mn = std::min(mm, nn);
        pack_core(h->stream, h, k, h->Wa);
        if ((rc = qr(h, mm, nn, h->Wa, s.Rm, s.tau))) return rc;
        hipLaunchKernelGGL(k_norm_log, dim3(1), dim3(1024), 0, h->stream, (size_t)mn * nn, s.Rm, s.acc, 1);
        unpack_core(h, k, h->Wa, r0, mn);
        push_right(h, k, s.Rm, mn);                                     // R pushed into the next core, fp64 MFMA
    }
    pack_core(h->stream, h, d, h->Wa);
    hipLaunchKernelGGL(k_norm_log, dim3(1), dim3(1024), 0, h->stream, core_elems(h, d), h->Wa, s.acc, 0);     // :184-188
    for (int k = 1; k <= d; k++)                                        // :190-194
        hipLaunchKernelGGL(k_scal_core_acc, g1(core_elems(h, k)), dim3(256), 0, h->stream, core_dev(h, k), r[k - 1], h->n1[k], r[k], h->RM, h->P.SS,
                           s.acc, d, (k == d) ? 1 : 0);
    push_ranks(h);
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}

// rank, Jacobi sweeps and singular values of the core just decomposed: written by the device into pinned memory, polled here
static int svd_fetch(ttx_engine *h, const double *sv, const int *info, int q, int *inf2, double *svh)
{
    if (!h->h_svd) { HIPCHECK(hipHostMalloc((void **)&h->h_svd, sizeof(double) * ((size_t)h->RM + 8))); h->h_svd[0] = 0.0; }
    if (env_off("TTX_SVD_POLL")) {
        HIPCHECK(hipMemcpyAsync(inf2, info, sizeof(int) * 2, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipMemcpyAsync(svh, sv, sizeof(double) * q, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        return TTX_OK;
    }
    h->svd_seq += 1.0;
    hipLaunchKernelGGL(k_svd_report, dim3(1), dim3(64), 0, h->stream, sv, info, q, (volatile double *)h->h_svd, h->svd_seq);
    HIPCHECK(hipGetLastError());
    volatile double *hv = h->h_svd;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (hv[0] != h->svd_seq) {
        if ((++spins & 0xfff) == 0) {
            if (hipStreamQuery(h->stream) == hipSuccess && hv[0] != h->svd_seq) {                   // (kernel failed to launch: do not spin for ever)
                HIPCHECK(hipStreamSynchronize(h->stream));
                if (hv[0] != h->svd_seq) return fail(TTX_EHIP, "dtt_svd: the device never reported rank and singular values");
                break;
            }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 30.0) return fail(TTX_EHIP, "dtt_svd: no report from the device within 30 s");
        }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    inf2[0] = (int)hv[1]; inf2[1] = (int)hv[2];
    for (int j = 0; j < q; j++) svh[j] = hv[3 + j];
    return TTX_OK;
}
static int svd_impl(ttx_engine *h, double tol, int rmax)
{
    const int d = h->d;
    if (d <= 1) return TTX_OK;
    int rc = ort_impl(h);
    if (rc) return rc;
    std::vector<int32_t> &r = h->rfinal;
    const TtScratch s(h);
    double lognrm = 0.0, s2;
    int e2 = 0;
    std::vector<double> svh(h->RM);
    for (int k = d; k >= 2; k--) {                                      // lib/tt.f90:329-356
        const int mm = r[k - 1], nn = h->n1[k] * r[k], q = std::min(mm, nn);
        // the unfolding A (mm x nn) of core k, with a q x q triangle X = Ub S Vb^T for the Jacobi step:
        //   tall (mm > nn, only possible for trains that do not come from a cross): A = Q R, X = R  =>  A = (Q Ub S) Vb^T
        //   wide: A^T = Q1 R1, X = R1^T                                                            =>  A = (Ub S) (Q1 Vb)^T
        const bool tall = mm > nn;
        double *X = tall ? s.Rm : s.Rt;
        pack_core(h->stream, h, k, h->Wa, tall ? 0 : 1);
        if ((rc = qr(h, std::max(mm, nn), q, h->Wa, s.Rm, s.tau))) return rc;   // Wa -> Q (mm x nn) or Q1 (nn x mm), Rm = R or R1
        if (!tall) hipLaunchKernelGGL(k_transpose, g1((size_t)mm * mm), dim3(256), 0, h->stream, mm, mm, s.Rm, s.Rt);
        if ((rc = jacobi(h, q, q, X, s.Vb, s.sv, s.perm, s.info, tol, rmax))) return rc;
        int inf[2];
        if ((rc = svd_fetch(h, s.sv, s.info, q, inf, svh.data()))) return rc;
        const int rr = inf[0];
        if (getenv("TTX_JAC_TRACE")) fprintf(stderr, "svd core %d: %d x %d, %d Jacobi sweeps, rank %d\n", k, q, q, inf[1], rr);
        const double nrm = host_norm(svh.data(), rr);
        if (nrm != 0.0) lognrm += std::log(nrm);
        take_cols(h, q, rr, X, s.perm, s.sv, nrm != 0.0 ? 1.0 / nrm : 1.0, s.US);
        if (tall) gemm(h, mm, rr, nn, h->Wa, mm, s.US, nn, h->Wd, mm);  // Q Ub S  (mm x rr)
        push_left(h, k, tall ? h->Wd : s.US, rr);                       // into the previous core
        take_cols(h, q, rr, s.Vb, s.perm, nullptr, 1.0, s.Vs);
        if (!tall) gemm(h, nn, rr, mm, h->Wa, nn, s.Vs, mm, h->Wd, nn); // Y = Q1 Vb(:, kept)  (nn x rr)
        unpack_core(h, k, tall ? s.Vs : h->Wd, rr, r[k], 1);            // the new core k is the transpose of Vb(:, kept) or of Y
        r[k - 1] = rr;
    }
    pack_core(h->stream, h, 1, h->Wa);
    if ((rc = sumsq(h, core_elems(h, 1), h->Wa, &s2, &e2))) return rc;
    double nf = std::ldexp(std::sqrt(s2), e2), firstscale = 1.0;
    if (nf != 0.0) { firstscale = 1.0 / nf; lognrm += std::log(nf); }
    lognrm /= d;
    const double nrm = std::exp(lognrm);
    for (int k = 1; k <= d; k++) scal_core(h, k, (k == 1) ? nrm * firstscale : nrm);
    push_ranks(h);
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}

// (ort / svd change the train in place: on a multi-process engine that would mean redistributing cores whose ranks have changed;
//  take a replica with ttx_replicate and work on that)
extern "C" int ttx_ort(ttx_engine *h) { int rc = tt_prepare(h, "dtt_ort"); return rc ? rc : ort_impl(h); }
extern "C" int ttx_svd(ttx_engine *h, double tol, int32_t rmax)
{
    if (!(tol >= 0.0)) return fail(TTX_EINVAL, "dtt_svd: tol must be a number >= 0 (got %g)", tol);
    if (rmax < 0) return fail(TTX_EINVAL, "dtt_svd: rmax must be >= 0 (0: absent; got %d)", (int)rmax);
    int rc = tt_prepare(h, "dtt_svd");
    return rc ? rc : svd_impl(h, tol, rmax);
}

// dtt_norm / dtt_lognrm: the norm of the core that carries it after svd (tol >= 0: core 1) or ort (tol < 0: core d), as sqrt(*s2) 2^*e
static int core_norm_impl(ttx_engine *h, double tol, double *s2_out, int *e_out, const char *who)
{
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    // the reference works on a copy (tmp = arg, lib/tt.f90:1082): back the cores and ranks up; they come back on every path out
    const size_t tot = (size_t)h->G * h->NC * h->P.CS;
    if (!h->bak) { if ((rc = dev_alloc(h, &h->bak, tot))) return rc; }
    HIPCHECK(hipMemcpyAsync(h->bak, h->P.arg, sizeof(double) * tot, hipMemcpyDeviceToDevice, h->stream));
    struct Restore {
        ttx_engine *h; size_t tot; std::vector<int32_t> ranks; bool done = false;
        int run()
        {
            done = true;
            const hipError_t e = hipMemcpyAsync(h->P.arg, h->bak, sizeof(double) * tot, hipMemcpyDeviceToDevice, h->stream);
            h->rfinal = ranks;
            push_ranks(h);
            HIPCHECK(e);
            return TTX_OK;
        }
        ~Restore() { if (!done) (void)run(); }
    } restore{h, tot, h->rfinal};
    const int kn = tol >= 0.0 ? 1 : h->d;
    if ((rc = tol >= 0.0 ? svd_impl(h, tol, 0) : ort_impl(h))) return rc;
    pack_core(h->stream, h, kn, h->Wa);
    rc = sumsq(h, core_elems(h, kn), h->Wa, s2_out, e_out);
    const int back = restore.run();
    return rc ? rc : back;
}
extern "C" int ttx_norm(ttx_engine *h, double tol, double *val)
{
    if (h && h->ran && h->W > 1) return with_replica(h, [&](ttx_engine *e) { return ttx_norm(e, tol, val); });
    if (!val) return fail(TTX_EINVAL, "dtt_norm: null result");
    double s2 = 0.0; int e = 0;
    if (int rc = core_norm_impl(h, tol, &s2, &e, "dtt_norm")) return rc;
    *val = std::pow(std::ldexp(std::sqrt(s2), e), h->d);               // :1089
    return TTX_OK;
}
extern "C" int ttx_lognrm(ttx_engine *h, double tol, double *val)
{
    if (h && h->ran && h->W > 1) return with_replica(h, [&](ttx_engine *e) { return ttx_lognrm(e, tol, val); });
    if (!val) return fail(TTX_EINVAL, "dtt_lognrm: null result");
    double s2 = 0.0; int e = 0;
    if (int rc = core_norm_impl(h, tol, &s2, &e, "dtt_lognrm")) return rc;
    *val = ((0.5 * std::log(s2) + e * std::log(2.0)) / std::log(10.0)) * h->d;    // :1114-1132, d log10 of the core's norm
    return TTX_OK;
}

extern "C" int ttx_dot(ttx_engine *x, ttx_engine *y, double *val)
{
    if (x && y && x->ran && y->ran && (x->W > 1 || y->W > 1)) {      // replicas of whichever train is spread over processes
        if (x->W > 1) return with_replica(x, [&](ttx_engine *ex) { return ttx_dot(ex, y, val); });
        return with_replica(y, [&](ttx_engine *ey) { return ttx_dot(x, ey, val); });
    }
    int rc = tt_prepare(x, "dtt_dot");
    if (rc || (rc = tt_prepare(y, "dtt_dot"))) return rc;
    if (!val) return fail(TTX_EINVAL, "dtt_dot: null result");
    if (x->d != y->d) return fail(TTX_EINVAL, "dtt_dot: dimensions not match");          // lib/tt.f90:1162
    for (int k = 1; k <= x->d; k++) if (x->n1[k] != y->n1[k]) return fail(TTX_EINVAL, "dtt_dot: sizes not match");
    if (x->cfg.device != y->cfg.device) return fail(TTX_EINVAL, "dtt_dot: both tensor trains must live on the same GPU");
    const int d = x->d;
    double *phi = TtScratch(x).Rm, *phi2 = TtScratch(x).Rt;           // the r x r interface matrices: rx*ry <= RM_x^2 is checked below
    const double one = 1.0;
    HIPCHECK(hipMemcpyAsync(phi, &one, sizeof(double), hipMemcpyHostToDevice, x->stream));
    HIPCHECK(hipStreamSynchronize(y->stream));
    for (int i = 1; i <= d; i++) {
        const int rx0 = x->rfinal[i - 1], rx1 = x->rfinal[i], ry0 = y->rfinal[i - 1], ry1 = y->rfinal[i], n = x->n1[i];
        // x's scratch holds: core i of y packed (ry0*n*ry1 -> Wb), phi*core (rx0*n*ry1 -> Wc), the interface matrices
        if ((size_t)rx1 * ry1 > (size_t)x->RM * x->RM || (size_t)rx0 * ry0 > (size_t)x->RM * x->RM || (size_t)rx0 * n * ry1 > x->P.CS ||
            (size_t)ry0 * n * ry1 > x->P.CS)
            return fail(TTX_EINVAL, "dtt_dot: ranks of y exceed the work space of x (call dot_product(y, x) or raise maxrank of x)");
        pack_core(x->stream, y, i, x->Wb);
        gemm(x, rx0, n * ry1, ry0, phi, rx0, x->Wb, ry0, x->Wc, rx0);                       // :1169
        pack_core(x->stream, x, i, x->Wa);
        hipLaunchKernelGGL(k_transpose, g1((size_t)rx0 * n * rx1), dim3(256), 0, x->stream, rx0 * n, rx1, x->Wa, x->Wd);
        gemm(x, rx1, ry1, rx0 * n, x->Wd, rx1, x->Wc, rx0 * n, phi2, rx1);                  // :1170
        std::swap(phi, phi2);
    }
    HIPCHECK(hipMemcpyAsync(val, phi, sizeof(double), hipMemcpyDeviceToHost, x->stream));
    HIPCHECK(hipStreamSynchronize(x->stream));
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}

// ztt_quad, the part both entry points share: the per-core matrices sum_j w(j) U_k(:, j, :) of cores lo..hi for nf weight vectors
struct ZquadStage { size_t lds; int *dr; double *dtq, *dout; };
static int zquad_stage(ttx_engine *h, int32_t nf, const double *w, int lo, int hi, DevTmp &tmp, ZquadStage &z)
{
    const int d = h->d, RM = h->RM;
    // the chain kernels keep two complex RM x RM matrices in LDS
    z.lds = sizeof(double) * 4 * (size_t)RM * RM;
    if (z.lds > TTX_LDS_DEVICE) return fail(TTX_EINVAL, "ztt_quad: maxrank %d needs %zu bytes of LDS for the chain (limit 160 KB, maxrank <= 71)", RM, z.lds);
    size_t sumn = 0;
    for (int k = 1; k <= d; k++) sumn += h->n1[k];
    std::vector<const double *> cp(d + 2, nullptr);
    for (int k = lo; k <= hi; k++) cp[k] = core_dev(h, k);
    const std::vector<int> rr(h->rfinal.begin(), h->rfinal.end());
    double *dw; const double **dcp;
    HIPCHECK(tmp.alloc(&dw, 2 * sumn * nf)); HIPCHECK(tmp.alloc(&z.dtq, (size_t)nf * (d + 1) * 2 * RM * RM));
    HIPCHECK(tmp.alloc(&z.dout, 2 * (size_t)nf)); HIPCHECK(tmp.alloc(&dcp, d + 2)); HIPCHECK(tmp.alloc(&z.dr, d + 1));
    HIPCHECK(hipMemcpy(dw, w, sizeof(double) * 2 * sumn * nf, hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(dcp, cp.data(), sizeof(double *) * (d + 2), hipMemcpyHostToDevice));
    HIPCHECK(hipMemcpy(z.dr, rr.data(), sizeof(int) * (d + 1), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_zquad_build, dim3(d, nf), dim3(256), 0, h->stream, d, RM, h->NM, h->P.SS, h->P.n, (const int *)z.dr, (const double *const *)dcp, (const double *)dw, 2 * sumn, z.dtq);
    return TTX_OK;
}
static int zquad_finish(ttx_engine *h, int32_t nf, const ZquadStage &z, double *out)
{
    HIPCHECK(hipMemcpyAsync(out, z.dout, sizeof(double) * 2 * nf, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
// ztt_quad of a MULTI-PROCESS job (lib/dmrgg.f90:1418-1523 is collective over mybonds): every process chains the matrices of the
// cores it holds, the partial products travel by a SUM all-reduce into zero-padded slots, every process folds them in rank order
static int zquad_multi(ttx_engine *h, int32_t nf, const double *w, double *out)
{
    if (!h->ran) return fail(TTX_ESTATE, "ztt_quad: run dtt_dmrgg first");
    HIPCHECK(hipSetDevice(h->cfg.device));
    const int d = h->d, RM = h->RM, W = h->W, nproc = h->cfg.nproc;
    auto lo_of = [&](int wr) { return h->own[(int)((long long)nproc * wr / W)]; };
    auto hi_of = [&](int wr) { const int ge = (int)((long long)nproc * (wr + 1) / W); return ge == nproc ? d : h->own[ge] - 1; };
    const int plo = lo_of(h->wrank), phi = hi_of(h->wrank);
    std::vector<int> dims(2 * W);
    for (int wr = 0; wr < W; wr++) { dims[2 * wr] = h->rfinal[lo_of(wr) - 1]; dims[2 * wr + 1] = h->rfinal[hi_of(wr)]; }
    DevTmp tmp;
    double *dpart; int *ddims;
    const size_t npart = (size_t)nf * W * 2 * RM * RM;
    HIPCHECK(tmp.alloc(&dpart, npart)); HIPCHECK(tmp.alloc(&ddims, 2 * (size_t)W));
    HIPCHECK(hipMemcpy(ddims, dims.data(), sizeof(int) * 2 * W, hipMemcpyHostToDevice));
    HIPCHECK(hipMemsetAsync(dpart, 0, sizeof(double) * npart, h->stream));
    ZquadStage z;
    int rc = zquad_stage(h, nf, w, plo, phi, tmp, z);
    if (rc) return rc;
    if ((rc = ensure_lds(h, reinterpret_cast<const void *>(k_zquad_chain_seg), z.lds)) || (rc = ensure_lds(h, reinterpret_cast<const void *>(k_zquad_fold), z.lds))) return rc;
    hipLaunchKernelGGL(k_zquad_chain_seg, dim3(nf), dim3(256), z.lds, h->stream, d, RM, (const int *)z.dr, (const double *)z.dtq, plo, phi, h->wrank, W, dpart);
    if ((rc = allreduce_big(h, dpart, npart))) return rc;
    hipLaunchKernelGGL(k_zquad_fold, dim3(nf), dim3(256), z.lds, h->stream, RM, W, (const int *)ddims, (const double *)dpart, z.dout);
    if ((rc = zquad_finish(h, nf, z, out))) return rc;
    if (h->cb_error) return fail(TTX_EHIP, "host transport: a sendrecv / allreduce callback failed");
    return TTX_OK;
}

extern "C" int ttx_zquad(ttx_engine *h, int32_t nf, const double *w, double *out)
{
    const bool multi = h && h->W > 1;
    if (!multi) if (int rc = tt_prepare(h, "ztt_quad")) return rc;
    if (nf < 1 || !w || !out) return fail(TTX_EINVAL, "ztt_quad: bad argument");
    if (multi) return zquad_multi(h, nf, w, out);
    DevTmp tmp;
    ZquadStage z;
    int rc = zquad_stage(h, nf, w, 1, h->d, tmp, z);
    if (rc || (rc = ensure_lds(h, reinterpret_cast<const void *>(k_zquad_chain), z.lds))) return rc;
    hipLaunchKernelGGL(k_zquad_chain, dim3(nf), dim3(256), z.lds, h->stream, h->d, h->RM, (const int *)z.dr, (const double *)z.dtq, z.dout);
    return zquad_finish(h, nf, z, out);
}

extern "C" int ttx_ijk(ttx_engine *h, const int32_t *ind, double *val)
{
    int rc = tt_prepare(h, "dtt_ijk");
    if (rc) return rc;
    if (!ind || !val) return fail(TTX_EINVAL, "dtt_ijk: null argument");
    const int d = h->d;
    for (int k = 1; k <= d; k++) if (ind[k - 1] <= 0 || ind[k - 1] > h->n1[k]) { *val = -3.0; return TTX_OK; }   // lib/tt.f90:639
    // x = U_d(:, ind_d, 1); for i = d-1..1: x = U_i(:, ind_i, :) x -- matrix-vector steps through the GEMM kernel
    double *xv = TtScratch(h).Rm, *zv = xv + h->RM;                   // two vectors of RM at the head of the scratch
    pack_core(h->stream, h, d, h->Wa);
    HIPCHECK(hipMemcpyAsync(xv, h->Wa + (size_t)h->rfinal[d - 1] * (ind[d - 1] - 1), sizeof(double) * h->rfinal[d - 1], hipMemcpyDeviceToDevice, h->stream));
    for (int i = d - 1; i >= 1; i--) {
        const int q0 = h->rfinal[i - 1], q1 = h->rfinal[i], n = h->n1[i];
        pack_core(h->stream, h, i, h->Wa);
        gemm(h, q0, 1, q1, h->Wa + (size_t)q0 * (ind[i - 1] - 1), q0 * n, xv, q1, zv, q0);
        std::swap(xv, zv);
    }
    HIPCHECK(hipMemcpyAsync(val, xv, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}

// ---- plumbing of the operations on the resident train: work space, tables, preflight --------------------------------------------
static int buf_reserve(ttx_engine *h, int slot, size_t bytes)
{
    EvBuf &b = h->scratch[slot];
    if (b.p && b.bytes >= bytes) return TTX_OK;
    if (b.p) { HIPCHECK(hipStreamSynchronize(h->stream)); (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    HIPCHECK(hipMalloc(&b.p, bytes + 64));
    b.bytes = bytes;
    return TTX_OK;
}
template <class T> static T *buf(ttx_engine *h, int slot) { return (T *)h->scratch[slot].p; }
// the slots a plan names, in its order; a plan gives 0 bytes to a slot its call does not use
struct SlotBytes { int slot; size_t bytes; };
static int buf_reserve(ttx_engine *h, std::initializer_list<SlotBytes> slots)
{
    for (const SlotBytes &s : slots) if (s.bytes) if (int rc = buf_reserve(h, s.slot, s.bytes)) return rc;
    return TTX_OK;
}
// the one place a launch's dynamic LDS goes above the default ceiling: where its plan says so
static int op_lds_raise(ttx_engine *h, const void *kernel, const OpLds &l) { return l.raise ? ensure_lds(h, kernel, l.bytes) : TTX_OK; }
// A plan's tier as the template argument of a launch: f(Tier<MR>()).  The kernels exist for MR = 1, 2, 4 and 8 (rank_tier); EVERY: for
// each MR of 1 .. 8 (k_bs_gemm)
template <int MR> using Tier = std::integral_constant<int, MR>;
template <bool EVERY = false, class F> static int with_tier(int tier, F f)
{
    if constexpr (EVERY) {
        if (tier == 3) return f(Tier<3>());
        if (tier == 5) return f(Tier<5>());
        if (tier == 6) return f(Tier<6>());
        if (tier == 7) return f(Tier<7>());
    }
    return tier == 1 ? f(Tier<1>()) : tier == 2 ? f(Tier<2>()) : tier == 4 ? f(Tier<4>()) : f(Tier<8>());
}
namespace {
// device image of a call's tables: arrays appended at 16-byte boundaries in a host vector of the engine, uploaded in one copy
struct OpMeta {
    std::vector<char> &host;
    explicit OpMeta(std::vector<char> &b) : host(b) { host.clear(); }
    template <class T> size_t put(const std::vector<T> &v)
    {
        const size_t off = (host.size() + 15) & ~(size_t)15;
        host.resize(off + sizeof(T) * std::max<size_t>(v.size(), 1));
        if (!v.empty()) memcpy(host.data() + off, v.data(), sizeof(T) * v.size());
        return off;
    }
    // the image into the slot, on the engine's stream; *base: where it starts on the device
    int upload(ttx_engine *h, int slot, char **base)
    {
        if (int rc = buf_reserve(h, slot, host.size())) return rc;
        *base = buf<char>(h, slot);
        HIPCHECK(hipMemcpyAsync(*base, host.data(), host.size(), hipMemcpyHostToDevice, h->stream));
        return TTX_OK;
    }
};
}
// points per chunk of a batched call, from the environment (read on every call) or the call's default
static size_t env_chunk(const char *name, size_t dflt)
{
    if (const char *e = getenv(name)) { const long long v = atoll(e); if (v >= 1) return (size_t)std::min<long long>(v, 1ll << 24); }
    return dflt;
}
static int dev_ncu(ttx_engine *h)
{
    if (!h->ncu) { h->ncu = 256; (void)hipDeviceGetAttribute(&h->ncu, hipDeviceAttributeMultiprocessorCount, h->cfg.device); }
    return h->ncu;
}
// the engines ttx_ijk takes: a train, one process (a multi-process engine gets tt_prepare's answer); makes its device current
static int check_train_one_process(ttx_engine *h, const char *who)
{
    if (!h || !h->ran) return fail(TTX_ESTATE, "%s: no tensor train (run dtt_dmrgg first)", who);
    if (h->W > 1) return tt_prepare(h, who);
    HIPCHECK(hipSetDevice(h->cfg.device));
    return TTX_OK;
}

// ---- TTX_FUN_TRAINS: operands, their device blocks, the list entry (kernels in ttx_trainfun.h) ------------------------------------
// one wave per item, TTX_TF_WAVES per workgroup, at most 8 workgroups per CU (the launch shape of k_ev_exact); the kernels stride
static int tf_grid(ttx_engine *h, long long items)
{
    return (int)std::max<long long>(1, std::min<long long>((items + TTX_TF_WAVES - 1) / TTX_TF_WAVES, (long long)dev_ncu(h) * 8));
}
// what an operand must be, for the set call and again before every evaluation (the caller may have changed it in between)
static int tf_check_operand(ttx_engine *h, ttx_engine *x, int t, const char *who)
{
    char w[160];
    snprintf(w, sizeof w, "%s: operand %d", who, t + 1);
    if (!x) return fail(TTX_EINVAL, "%s is null", w);
    if (x == h) return fail(TTX_EINVAL, "%s is the engine itself: its train is what the run writes", w);
    if (int rc = check_train_one_process(x, w)) return rc;
    if (x->cfg.device != h->cfg.device) return fail(TTX_EINVAL, "%s lives on device %d, the engine on device %d", w, x->cfg.device, h->cfg.device);
    if (x->d != h->d) return fail(TTX_EINVAL, "%s has %d modes, the engine %d", w, x->d, h->d);
    for (int k = 1; k <= h->d; k++) if (x->n1[k] != h->n1[k]) return fail(TTX_EINVAL, "%s: mode %d has %d points, the engine's %d", w, k, x->n1[k], h->n1[k]);
    for (int k = 0; k <= h->d; k++) if (x->rfinal[k] < 1 || x->rfinal[k] > 128) return fail(TTX_EINVAL, "%s: rank %d at bond %d (1..128 expected)", w, x->rfinal[k], k);
    if (x->rfinal[0] != 1 || x->rfinal[h->d] != 1) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", w);
    return TTX_OK;
}
// The operands' blocks -- core pointers and ranks of every operand as they stand NOW, the engine's mode sizes -- into this engine's
// own scratch (SC_TFUN), so that an operand that was ort-ed or svd-ed since the last run is seen with its new ranks and stays free
// for calls of its own between runs.  One wait: the operands' streams have finished what wrote their cores, the engine's stream has
// the blocks.  The counter of evaluated elements (SC_CNT) and, for a loaded combiner, the value rows (SC_TVAL) are made ready too.
// figures: the call records what ttx_trainfun_last reports (ttx_accchk leaves the last run's figures as they are).
static int tf_prepare(ttx_engine *h, const char *who, bool figures)
{
    if (!h->tfun) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_trains first", who);
    const TrainFun &f = *h->tfun;
    const int m = (int)f.x.size(), d = h->d;
    for (int t = 0; t < m; t++) if (int rc = tf_check_operand(h, f.x[t], t, who)) return rc;
    HIPCHECK(hipSetDevice(h->cfg.device));
    OpMeta meta(h->tf_host);
    size_t o_core[TTX_TF_MAX], o_r[TTX_TF_MAX];
    int rmax = 1;
    for (int t = 0; t < m; t++) {
        const ttx_engine *x = f.x[t];
        std::vector<const double *> cp(d);
        for (int k = 1; k <= d; k++) cp[k - 1] = core_dev(x, k);
        const std::vector<int> r(x->rfinal.begin(), x->rfinal.begin() + d + 1);
        rmax = std::max(rmax, *std::max_element(r.begin(), r.end()));
        o_core[t] = meta.put(cp); o_r[t] = meta.put(r);
    }
    const size_t o_n = meta.put(std::vector<int>(h->n1.begin() + 1, h->n1.begin() + 1 + d));
    for (int t = 0; t < m; t++) HIPCHECK(hipStreamSynchronize(f.x[t]->stream));
    char *dm;
    int rc;
    if ((rc = meta.upload(h, SC_TFUN, &dm)) || (rc = buf_reserve(h, SC_CNT, sizeof(long long)))) return rc;
    if (f.op == TTX_TOP_DEVICE && (rc = buf_reserve(h, SC_TVAL, sizeof(double) * (size_t)h->G * h->sel.HS * m))) return rc;
    HIPCHECK(hipMemsetAsync(buf<char>(h, SC_CNT), 0, sizeof(long long), h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    TfOps &O = h->tf_ops;
    O = TfOps{};
    O.m = m; O.d = d; O.ldx = (rmax + 3) & ~3; O.n = (const int *)(dm + o_n);
    for (int t = 0; t < m; t++) {
        O.t[t].RM = f.x[t]->RM; O.t[t].SS = f.x[t]->P.SS;
        O.t[t].core = (const double *const *)(dm + o_core[t]); O.t[t].r = (const int *)(dm + o_r[t]);
    }
    h->tf_figures = figures;
    if (!figures) return TTX_OK;
    h->tf_launches = 0; h->tf_elements = 0; h->tf_ms = 0.0;
    for (auto &e : h->tf_evs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    h->tf_evs.clear();
    return TTX_OK;
}
// after the last launch of a call: the elements the slot kernel evaluated and, with ttx_set_profile on, its milliseconds
static int tf_finish(ttx_engine *h)
{
    unsigned long long c = 0;
    HIPCHECK(hipMemcpyAsync(&c, buf<char>(h, SC_CNT), sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->tf_elements = (int64_t)c;
    for (auto &e : h->tf_evs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) h->tf_ms += ms;
        (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    h->tf_evs.clear();
    return TTX_OK;
}
static int tf_set(const char *who, ttx_engine *h, int32_t m, ttx_engine *const *x, int32_t op, std::shared_ptr<DevFun> comb)
{
    if (m < 1 || m > TTX_TRAINS_MAX) return fail(TTX_EINVAL, "%s: %d operands (1..%d expected)", who, m, TTX_TRAINS_MAX);
    if (!x) return fail(TTX_EINVAL, "%s: operand list missing", who);
    if (op < TTX_TOP_PRODUCT || op > TTX_TOP_DEVICE) return fail(TTX_EINVAL, "%s: unknown op %d", who, op);
    if (op == TTX_TOP_RATIO && m != 2) return fail(TTX_EINVAL, "%s: TTX_TOP_RATIO takes 2 operands (got %d)", who, m);
    if (op == TTX_TOP_SQRTABS && m != 1) return fail(TTX_EINVAL, "%s: TTX_TOP_SQRTABS takes 1 operand (got %d)", who, m);
    for (int t = 0; t < m; t++) if (int rc = tf_check_operand(h, x[t], t, who)) return rc;
    HIPCHECK(hipSetDevice(h->cfg.device));
    auto f = std::make_shared<TrainFun>();
    f->x.assign(x, x + m); f->op = op; f->comb = std::move(comb);
    HIPCHECK(hipStreamSynchronize(h->stream));          // nothing of an earlier combiner is in flight when its module goes
    h->tfun = std::move(f);
    return TTX_OK;
}
extern "C" int ttx_set_integrand_trains(ttx_engine *h, int32_t m, ttx_engine *const *x, int32_t op)
{
    const char *who = "ttx_set_integrand_trains";
    if (!h) return fail(TTX_EINVAL, "%s: null handle", who);
    if (h->cfg.fun_id != TTX_FUN_TRAINS) return fail(TTX_ESTATE, "%s: the engine was not created with fun_id = TTX_FUN_TRAINS", who);
    if (op == TTX_TOP_DEVICE) return fail(TTX_EINVAL, "%s: TTX_TOP_DEVICE needs a code object: ttx_set_integrand_trains_device", who);
    return tf_set(who, h, m, x, op, nullptr);
}
extern "C" int ttx_set_integrand_trains_device(ttx_engine *h, int32_t m, ttx_engine *const *x, const void *image, int64_t nbytes,
                                               const char *name, const double *par, int32_t npar)
{
    const char *who = "ttx_set_integrand_trains_device";
    if (!h) return fail(TTX_EINVAL, "%s: null handle", who);
    if (h->cfg.fun_id != TTX_FUN_TRAINS) return fail(TTX_ESTATE, "%s: the engine was not created with fun_id = TTX_FUN_TRAINS", who);
    if (m < 1 || m > TTX_TRAINS_MAX) return fail(TTX_EINVAL, "%s: %d operands (1..%d expected)", who, m, TTX_TRAINS_MAX);
    if (!x) return fail(TTX_EINVAL, "%s: operand list missing", who);
    for (int t = 0; t < m; t++) if (int rc = tf_check_operand(h, x[t], t, who)) return rc;     // before the code object is loaded
    std::shared_ptr<DevFun> c;
    if (int rc = devfun_load(who, "ttx_devcomb_", "TTX_DEVICE_COMBINER", "combiner", h, image, nbytes, name, par, npar, &c)) return rc;
    if (c->info.kind != TTX_DEVFUN_KIND_LANE) return fail(TTX_EINVAL, "%s: combiner '%s' is not of the lane form", who, name);
    return tf_set(who, h, m, x, TTX_TOP_DEVICE, std::move(c));
}
extern "C" int ttx_set_integrand_trains_device_file(ttx_engine *h, int32_t m, ttx_engine *const *x, const char *path, const char *name,
                                                    const double *par, int32_t npar)
{
    const char *who = "ttx_set_integrand_trains_device_file";
    if (!h) return fail(TTX_EINVAL, "%s: null handle", who);
    if (h->cfg.fun_id != TTX_FUN_TRAINS) return fail(TTX_ESTATE, "%s: the engine was not created with fun_id = TTX_FUN_TRAINS", who);
    std::vector<unsigned char> img;
    std::string text;
    if (int rc = devfun_read_file(who, path, img, &text)) return fail(rc, "%s", text.c_str());
    return ttx_set_integrand_trains_device(h, m, x, img.data(), (int64_t)img.size(), name, par, npar);
}
extern "C" int ttx_trainfun_last(const ttx_engine *h, double *ms, int64_t *launches, int64_t *elements)
{
    if (!h) return fail(TTX_EINVAL, "ttx_trainfun_last: null handle");
    if (ms) *ms = h->tf_ms;
    if (launches) *launches = h->tf_launches;
    if (elements) *elements = h->tf_elements;
    return TTX_OK;
}
// ttx_eval_device of a TTX_FUN_TRAINS engine: k_tf_list over the staged rows, in chunks; a loaded combiner's list kernel behind it
static int tf_eval_list(ttx_engine *h, int64_t npts, const int32_t *ind, double *out)
{
    if (npts < 0 || (npts > 0 && (!ind || !out))) return fail(TTX_EINVAL, "ttx_eval_device: null argument");
    int rc = tf_prepare(h, "ttx_eval_device", true);
    if (rc) return rc;
    if (npts == 0) return TTX_OK;
    const int d = h->d;
    for (int64_t p = 0; p < npts; p++)
        for (int k = 0; k < d; k++)
            if (ind[p * d + k] < 1 || ind[p * d + k] > h->n1[k + 1])
                return fail(TTX_EINVAL, "ttx_eval_device: point %lld: index %d of mode %d is outside 1..%d", (long long)p, ind[p * d + k], k + 1, h->n1[k + 1]);
    const TrainFun &f = *h->tfun;
    const TfOps &O = h->tf_ops;
    const size_t chunk = (size_t)std::min<int64_t>(npts, 1 << 16);
    if ((rc = buf_reserve(h, SC_IND, sizeof(int) * chunk * d)) || (rc = buf_reserve(h, SC_OUT, sizeof(double) * chunk))) return rc;
    if (f.op == TTX_TOP_DEVICE && (rc = buf_reserve(h, SC_TVAL, sizeof(double) * std::max(chunk, (size_t)h->G * h->sel.HS) * O.m))) return rc;
    int *sind = buf<int>(h, SC_IND);
    double *sout = buf<double>(h, SC_OUT), *tval = buf<double>(h, SC_TVAL);
    unsigned long long *cnt = buf<unsigned long long>(h, SC_CNT);
    const size_t lds = sizeof(double) * TTX_TF_WAVES * tf_lds_doubles(O.ldx, O.d);
    const dim3 block(64 * TTX_TF_WAVES);
    for (int64_t o = 0; o < npts; o += (int64_t)chunk) {
        long long c = std::min<int64_t>((int64_t)chunk, npts - o);
        const dim3 grid(tf_grid(h, c));
        HIPCHECK(hipMemcpyAsync(sind, ind + (size_t)o * d, sizeof(int) * (size_t)c * d, hipMemcpyHostToDevice, h->stream));
        h->tf_launches++;
        {
            TfScope timed(h);
            switch (f.op) {
                case TTX_TOP_PRODUCT: hipLaunchKernelGGL(k_tf_list<TF_PRODUCT>, grid, block, lds, h->stream, O, c, (const int *)sind, sout, tval, cnt); break;
                case TTX_TOP_RATIO: hipLaunchKernelGGL(k_tf_list<TF_RATIO>, grid, block, lds, h->stream, O, c, (const int *)sind, sout, tval, cnt); break;
                case TTX_TOP_SQRTABS: hipLaunchKernelGGL(k_tf_list<TF_SQRTABS>, grid, block, lds, h->stream, O, c, (const int *)sind, sout, tval, cnt); break;
                default: {
                    hipLaunchKernelGGL(k_tf_list<TF_DEVICE>, grid, block, lds, h->stream, O, c, (const int *)sind, sout, tval, cnt);
                    DevFun &cb = *f.comb;
                    int m = O.m, dd = d;
                    const int *n = h->P.n + 1, *ip = sind;
                    const double *par = cb.par, *tv = tval;
                    const unsigned cg = (unsigned)std::max<long long>(1, std::min<long long>((c + cb.info.block - 1) / cb.info.block, 4096));
                    void *args[] = {&m, &dd, &n, &par, &c, &ip, &tv, &sout};
                    DEVFUN_LAUNCHCHECK(hipModuleLaunchKernel(cb.list, cg, 1, 1, (unsigned)cb.info.block, 1, 1, 0, h->stream, args, nullptr));
                }
            }
        }
        HIPCHECK(hipMemcpyAsync(out + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    HIPCHECK(hipGetLastError());
    return tf_finish(h);
}

// ---- the train at a batch of multi-indices (ttx_eval.h) -------------------------------------------------------------------------
// core pointers, ranks and mode sizes of the train as it stands now, in one device block
static int ev_train(ttx_engine *h, EvTrain *T)
{
    const int d = h->d;
    std::vector<const double *> cp(d);
    std::vector<int> r(h->rfinal.begin(), h->rfinal.begin() + d + 1), n(h->n1.begin() + 1, h->n1.begin() + 1 + d);
    for (int k = 1; k <= d; k++) cp[k - 1] = core_dev(h, k);
    const int rmax = std::max(1, *std::max_element(r.begin(), r.end()));
    if (rmax > 128) return fail(TTX_EINVAL, "ttx_ijk_batch: ranks up to 128 only (got %d)", rmax);      // kept: this name, whichever entry called
    OpMeta meta(h->train_host);
    const size_t o_core = meta.put(cp), o_r = meta.put(r), o_n = meta.put(n);
    char *m;
    if (int rc = meta.upload(h, SC_TRAIN, &m)) return rc;
    T->d = d; T->RM = h->RM; T->ldx = (rmax + 3) & ~3; T->SS = h->P.SS;
    T->core = (const double *const *)(m + o_core); T->r = (const int *)(m + o_r); T->n = (const int *)(m + o_n);
    return TTX_OK;
}
static EvPlan ev_plan(ttx_engine *h, EvStage st, int64_t npts, int32_t dd, int32_t mode)
{
    return ev_plan(h->d, h->n1.data() + 1, h->rfinal.data(), h->NM, dev_ncu(h), st, npts, dd, mode, env_chunk("TTX_IJK_CHUNK", op_chunk_default(h->RM)));
}
// c points whose index rows (and, for ttx_value_batch, flags) are on the device -> out (device), enqueued on the engine's stream
static int ev_run(ttx_engine *h, const EvPlan &pl, const EvTrain &T, int c, const int *ind, const int *flag, double *out)
{
    const int d = h->d;
    if (pl.eff == TTX_EVAL_EXACT) {
        // the grid strides over the batch (66 VGPRs: 7 waves per SIMD are resident); the chain is a dependent sequence, throughput
        // comes from the waves in flight
        hipLaunchKernelGGL(k_ev_exact, dim3(pl.g_wave(c)), dim3(256), pl.exact_lds, h->stream, T, (long long)c, ind, flag, out);
        return TTX_OK;
    }
    const size_t NM = h->NM;
    double *X = buf<double>(h, SC_XA), *Z = buf<double>(h, SC_XB);
    int *valid = buf<int>(h, SC_SORT), *perm = valid + c, *cnt = perm + c, *off = cnt + NM, *tile = off + NM + 1, *cur = tile + NM + 1;
    hipLaunchKernelGGL(k_ev_init, dim3(pl.g_wave(c)), dim3(256), 0, h->stream, T, c, ind, flag, valid, X, out);
    const int nb = pl.g_sort(c);
    for (int i = d - 2; i >= 0; i--) {
        const EvStep &s = pl.step[i];
        HIPCHECK(hipMemsetAsync(cnt, 0, sizeof(int) * s.nmode, h->stream));
        hipLaunchKernelGGL(k_ev_hist, dim3(nb), dim3(256), s.hist_lds, h->stream, d, i, s.nmode, c, ind, (const int *)valid, cnt);
        hipLaunchKernelGGL(k_ev_scan, dim3(1), dim3(1024), 0, h->stream, s.nmode, (const int *)cnt, off, tile, cur);
        hipLaunchKernelGGL(k_ev_scatter, dim3(nb), dim3(256), s.hist_lds, h->stream, d, i, s.nmode, c, ind, (const int *)valid, cur, perm);
        if (int rc = with_tier(s.tier, [&](auto mr) {
                constexpr int MR = decltype(mr)::value;
                if (int rc = op_lds_raise(h, reinterpret_cast<const void *>(k_ev_gemm<MR>), s.lds)) return rc;
                hipLaunchKernelGGL(k_ev_gemm<MR>, dim3(pl.g_gemm(i, c)), dim3(256), s.lds.bytes, h->stream, T, i, s.nmode, (const int *)off, (const int *)tile, (const int *)perm,
                                   (const double *)X, Z);
                return (int)TTX_OK;
            })) return rc;
        std::swap(X, Z);
    }
    hipLaunchKernelGGL(k_ev_final, dim3(pl.g_final(c)), dim3(256), 0, h->stream, c, T.ldx, (const int *)valid, (const double *)X, out);
    return TTX_OK;
}
extern "C" int ttx_eval_last_mode(const ttx_engine *h) { return h ? h->ev_last_mode : -1; }

// the three entries differ in where a chunk's index rows come from and where its values go (EvStage)
// `in`: npts x d index rows (int32) or, EV_HOST_COORD, npts x dd coordinates (double); lib/tt.f90:702-728 forms the digits, then dtt_ijk
static int ev_batch(ttx_engine *h, const char *who, EvStage st, int64_t npts, int32_t dd, const void *in, double *out, int32_t mode)
{
    int rc = tt_prepare(h, st == EV_HOST_COORD ? "dtt_value" : "dtt_ijk");
    if (rc) return rc;
    if (npts < 0 || (npts > 0 && (!in || !out))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if (st == EV_HOST_COORD && dd < 1) return fail(TTX_EINVAL, "%s: %d coordinates per point", who, dd);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    const EvPlan pl = ev_plan(h, st, npts, dd, mode);
    // an asymmetry of the entries, kept: an empty ttx_value_batch leaves ev_last_mode as it was, the two index entries record theirs
    if (npts == 0) { if (st != EV_HOST_COORD) h->ev_last_mode = pl.eff; return TTX_OK; }
    const int32_t *ind = (const int32_t *)in;
    const double *x = (const double *)in;
    // int(xx) of the reference is defined below 2^31 only
    if (st == EV_HOST_COORD)
        for (size_t e = 0; e < (size_t)npts * dd; e++) if (!(x[e] < 2147483648.0)) return fail(TTX_EINVAL, "%s: coordinate %g of point %lld is not below 2^31", who, x[e], (long long)(e / dd));
    EvTrain T;
    if ((rc = ev_train(h, &T)) ||
        (rc = buf_reserve(h, {{SC_IND, pl.b_ind}, {SC_OUT, pl.b_out}, {SC_FLAG, pl.b_flag}, {SC_X, pl.b_x}, {SC_XA, pl.b_xa}, {SC_XB, pl.b_xb}, {SC_SORT, pl.b_sort}}))) return rc;
    const size_t d = h->d;
    int *sind = buf<int>(h, SC_IND), *sflag = st == EV_HOST_COORD ? buf<int>(h, SC_FLAG) : nullptr;
    double *sout = buf<double>(h, SC_OUT), *sx = buf<double>(h, SC_X);
    for (int64_t o = 0; o < npts; o += (int64_t)pl.chunk) {
        const int c = (int)std::min<int64_t>((int64_t)pl.chunk, npts - o);
        if (st == EV_ON_DEVICE) {
            if ((rc = ev_run(h, pl, T, c, ind + (size_t)o * d, nullptr, out + o))) return rc;
            continue;                                                           // one wait after the last chunk
        }
        if (st == EV_HOST_INDEX) HIPCHECK(hipMemcpyAsync(sind, ind + (size_t)o * d, sizeof(int) * (size_t)c * d, hipMemcpyHostToDevice, h->stream));
        else {
            HIPCHECK(hipMemcpyAsync(sx, x + (size_t)o * dd, sizeof(double) * (size_t)c * dd, hipMemcpyHostToDevice, h->stream));
            hipLaunchKernelGGL(k_ev_digits, g1((size_t)c), dim3(256), 0, h->stream, (int)d, T.n, (int)dd, (long long)c, (const double *)sx, sind, sflag);
        }
        if ((rc = ev_run(h, pl, T, c, sind, sflag, sout))) return rc;
        HIPCHECK(hipMemcpyAsync(out + o, sout, sizeof(double) * c, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));                              // the staging blocks are reused by the next chunk
    }
    if (st == EV_ON_DEVICE) HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    h->ev_last_mode = pl.eff;
    return TTX_OK;
}
extern "C" int ttx_ijk_batch_dev(ttx_engine *h, int64_t npts, const int32_t *ind_dev, double *out_dev, int32_t mode)
{
    return ev_batch(h, "ttx_ijk_batch_dev", EV_ON_DEVICE, npts, 0, ind_dev, out_dev, mode);
}
extern "C" int ttx_ijk_batch(ttx_engine *h, int64_t npts, const int32_t *ind, double *out, int32_t mode)
{
    return ev_batch(h, "ttx_ijk_batch", EV_HOST_INDEX, npts, 0, ind, out, mode);
}
// dtt_value for npts coordinate vectors of dd entries each
extern "C" int ttx_value_batch(ttx_engine *h, int64_t npts, int32_t dd, const double *x, double *out, int32_t mode)
{
    return ev_batch(h, "ttx_value_batch", EV_HOST_COORD, npts, dd, x, out, mode);
}

extern "C" int ttx_arith(const ttx_engine *h) { return h ? h->arith() : -1; }
extern "C" int ttx_sweep_path(const ttx_engine *h) { return !h ? -1 : h->cluster_nb() ? 2 : h->sel.fused ? 1 : 0; }
extern "C" int64_t ttx_resid_halfsteps(const ttx_engine *h) { return h ? h->n_resid : 0; }
extern "C" int ttx_cluster_eval(const ttx_engine *h) { return !h ? -1 : h->cluster_nb() ? 1 + h->sel.cluster_var : 0; }
extern "C" int ttx_cluster_fallbacks(const ttx_engine *h) { return h ? h->cluster_fallbacks : 0; }
extern "C" int ttx_cluster_entry(const ttx_engine *h, int64_t out[3])
{
    if (!h || !out) return fail(TTX_EINVAL, "ttx_cluster_entry: null argument");
    out[0] = out[1] = out[2] = 0;
    if (!h->cluster_nb()) return TTX_OK;
    const CreatePlan &s = h->sel;
    out[0] = (s.cl_powtab ? 1 : 0) | (s.cl_word ? 2 : 0) | (s.cl_lists ? 4 : 0);
    GroupState g0s;
    HIPCHECK(hipSetDevice(h->cfg.device));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipMemcpy(&g0s, h->P.gs, offsetof(GroupState, S), hipMemcpyDeviceToHost));
    out[1] = g0s.n_zload; out[2] = g0s.n_wload;
    return TTX_OK;
}
extern "C" int ttx_sweep_gap(const ttx_engine *h, int32_t out[4])
{
    if (!h || !out) return fail(TTX_EINVAL, "ttx_sweep_gap: null argument");
    const CreatePlan &s = h->sel;
    out[0] = (s.tail_event_kernel && !h->tail_event_retired) ? 1 : 0; out[1] = h->tail_event_fallbacks;
    out[2] = s.tail_lean ? 1 : 0; out[3] = s.cl_pack2 ? 1 : 0;
    return TTX_OK;
}
extern "C" int ttx_det_fallbacks(const ttx_engine *h) { return h ? h->det_fallbacks + h->de5_fallbacks : 0; }
extern "C" int ttx_fun_id(const ttx_engine *h) { return h ? h->cfg.fun_id : -1; }
extern "C" int ttx_set_profile(ttx_engine *h, int on) { if (!h) return fail(TTX_EINVAL, "null"); h->profile = on != 0; return TTX_OK; }
// ---- chosen modes contracted with rank-1 weights (ttx_contract.h) ---------------------------------------------------------------
// the plan of all modes (ttx_op_plan.h) with the cores' addresses as they stand now
static void ct_plan(ttx_engine *h, const std::vector<char> &contracted, CtPlan &pl)
{
    ct_plan(h->d, h->n1.data() + 1, h->rfinal.data(), contracted, pl);
    for (int k = 0; k < h->d; k++) pl.cores[k].src = core_dev(h, k + 1);
}
// weights to the device (NULL: ones) and the mode-sum launch, between the timer's events where the caller reports its time
static int ct_modesum(ttx_engine *h, const CtPlan &pl, const double *w, const CtCore *dcores, const CtTile *dtiles, OpTimer *tm)
{
    int rc;
    if ((rc = buf_reserve(h, SC_W, sizeof(double) * pl.wsize)) || (rc = buf_reserve(h, SC_M, sizeof(double) * std::max<size_t>(pl.msize, 1)))) return rc;
    std::vector<double> ones;
    if (!w) { ones.assign(pl.wsize, 1.0); w = ones.data(); }
    HIPCHECK(hipMemcpyAsync(buf<double>(h, SC_W), w, sizeof(double) * pl.wsize, hipMemcpyHostToDevice, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));                                  // `ones` leaves scope
    if (pl.tiles.empty()) return TTX_OK;
    if (tm && (rc = tm->start(h->stream))) return rc;
    hipLaunchKernelGGL(k_ct_modesum, dim3((unsigned)pl.tiles.size()), dim3(256), 0, h->stream, dcores, dtiles, h->RM, h->P.SS,
                       (const double *)buf<double>(h, SC_W), buf<double>(h, SC_M));
    return tm ? tm->stop(h->stream) : TTX_OK;
}
// the end of ttx_contract and ttx_marginals: the wait, then the figures of ttx_contract_modesum
static int ct_finish(ttx_engine *h, const CtPlan &pl)
{
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    h->ct = CtLast{0.0, pl.bytes};
    return pl.tiles.empty() ? TTX_OK : h->timer[TM_MODESUM].ms(&h->ct.ms);
}
// everything of ttx_contract that works on the new engine e: a failure leaves e to the caller to destroy
static int ct_fill(ttx_engine *h, ttx_engine *e, const std::vector<int> &kept, const double *w)
{
    const int d = h->d, m = (int)kept.size();
    std::vector<char> contracted(d, 1);
    for (int k : kept) contracted[k] = 0;
    CtPlan pl;
    ct_plan(h, contracted, pl);
    const std::vector<int> &r = pl.r;
    // maximal runs of contracted modes: before the first kept mode, between two kept modes, after the last
    std::vector<CtRun> runs;
    std::vector<int> run_left(m, -1);           // run ending just before kept mode j
    int run_trail = -1;
    size_t psize = 0, ssize = 0;
    for (int j = 0; j <= m; j++) {
        const int a = j ? kept[j - 1] + 1 : 0, b = (j < m ? kept[j] : d) - 1;
        if (b < a) continue;
        CtRun R{};
        R.k0 = a; R.cnt = b - a + 1; R.kind = j == 0 ? 0 : j == m ? 1 : 2; R.wmax = 1;
        for (int k = a; k <= b; k++) R.wmax = std::max(R.wmax, r[k + 1]);
        R.poff = psize; R.soff = ssize;
        psize += R.kind == 2 ? (size_t)r[a] * r[b + 1] : R.kind == 0 ? (size_t)r[b + 1] : (size_t)r[a];
        if (R.kind == 2 && 2 * (size_t)r[a] * R.wmax > TTX_CT_LDS) ssize += 2 * (size_t)r[a] * R.wmax;
        if (j < m) run_left[j] = (int)runs.size(); else run_trail = (int)runs.size();
        runs.push_back(R);
    }
    int rc;
    if ((rc = buf_reserve(h, SC_P, sizeof(double) * std::max<size_t>(psize, 1))) ||
        (rc = buf_reserve(h, SC_SCR, sizeof(double) * std::max<size_t>(ssize, 1)))) return rc;
    const double *Pb = buf<double>(h, SC_P);
    std::vector<CtKeep> keeps(m);
    long long items = 0;
    for (int j = 0; j < m; j++) {
        const int k = kept[j];
        CtKeep &K = keeps[j];
        K.src = pl.cores[k].src; K.dst = core_dev(e, j + 1);
        K.r0 = r[k]; K.n = h->n1[k + 1]; K.r1 = r[k + 1];
        K.P = run_left[j] >= 0 ? Pb + runs[run_left[j]].poff : nullptr;
        K.q0 = run_left[j] >= 0 ? r[runs[run_left[j]].k0] : K.r0;
        K.t = (j == m - 1 && run_trail >= 0) ? Pb + runs[run_trail].poff : nullptr;
        K.ncol = (K.n + 15) / 16; K.first = items; K.pad = 0;
        items += (long long)K.ncol * (K.t ? 1 : K.r1);
    }
    if (items > 0x7fffffffll) return fail(TTX_EINVAL, "ttx_contract: too many column tiles (%lld)", items);
    OpMeta meta(h->meta_host);
    const size_t o_cores = meta.put(pl.cores), o_tiles = meta.put(pl.tiles), o_runs = meta.put(runs), o_r = meta.put(r), o_moff = meta.put(pl.moff), o_keeps = meta.put(keeps);
    char *dm;
    if ((rc = meta.upload(h, SC_META, &dm)) ||
        (rc = ct_modesum(h, pl, w, (const CtCore *)(dm + o_cores), (const CtTile *)(dm + o_tiles), &h->timer[TM_MODESUM]))) return rc;
    if (!runs.empty())
        hipLaunchKernelGGL(k_ct_runs, dim3((unsigned)runs.size()), dim3(1024), 0, h->stream, (const CtRun *)(dm + o_runs), (const int *)(dm + o_r), (const size_t *)(dm + o_moff),
                           (const double *)buf<double>(h, SC_M), buf<double>(h, SC_P), buf<double>(h, SC_SCR));
    hipLaunchKernelGGL(k_ct_absorb, dim3((unsigned)items), dim3(64), 0, h->stream, (const CtKeep *)(dm + o_keeps), m, h->RM, h->P.SS, e->RM, e->P.SS);
    return ct_finish(h, pl);
}
extern "C" int ttx_contract(ttx_engine *h, const int32_t *keep, const double *w, ttx_engine **out)
{
    if (out) *out = nullptr;
    if (!keep || !out) return fail(TTX_EINVAL, "ttx_contract: null argument");
    int rc = check_train_one_process(h, "ttx_contract");
    if (rc) return rc;
    const int d = h->d;
    std::vector<int> kept;
    for (int k = 0; k < d; k++) {
        if (keep[k] != 0 && keep[k] != 1) return fail(TTX_EINVAL, "ttx_contract: keep(%d) = %d (0 or 1 expected)", k + 1, keep[k]);
        if (keep[k]) kept.push_back(k);
    }
    const int m = (int)kept.size();
    if (m < 2) return fail(TTX_EINVAL, "ttx_contract: %d kept mode%s, but the engine holds trains of at least two cores: ttx_marginals gives the one-mode marginals, ttx_quad the full sum", m, m == 1 ? "" : "s");
    // new ranks: r'(0) = 1, r'(j) = r(k_j) for j < m, r'(m) = 1
    std::vector<int32_t> nn(m), rr(m + 1, 1);
    for (int j = 0; j < m; j++) { nn[j] = h->n1[kept[j] + 1]; if (j < m - 1) rr[j + 1] = h->rfinal[kept[j] + 1]; }
    rr[0] = kept[0] == 0 ? h->rfinal[0] : 1; rr[m] = kept[m - 1] == d - 1 ? h->rfinal[d] : 1;
    return new_train(out, "ttx_contract", m, nn.data(), rr.data(), h->cfg.device, [&](ttx_engine *e) { return ct_fill(h, e, kept, w); });
}
extern "C" int ttx_marginals(ttx_engine *h, const double *w, double *out)
{
    if (!out) return fail(TTX_EINVAL, "ttx_marginals: null argument");
    int rc = check_train_one_process(h, "ttx_marginals");
    if (rc) return rc;
    const int d = h->d;
    CtPlan pl;
    ct_plan(h, std::vector<char>(d, 1), pl);
    const int ldv = h->RM;
    OpMeta meta(h->meta_host);
    const size_t o_cores = meta.put(pl.cores), o_tiles = meta.put(pl.tiles), o_r = meta.put(pl.r), o_moff = meta.put(pl.moff);
    char *dm;
    if ((rc = meta.upload(h, SC_META, &dm)) || (rc = buf_reserve(h, SC_VEC, sizeof(double) * (2 * (size_t)d + 4) * ldv)) ||
        (rc = buf_reserve(h, SC_OUT, sizeof(double) * pl.wsize)) ||
        (rc = ct_modesum(h, pl, w, (const CtCore *)(dm + o_cores), (const CtTile *)(dm + o_tiles), &h->timer[TM_MODESUM]))) return rc;
    double *L = buf<double>(h, SC_VEC), *S = L + (size_t)d * ldv, *dout = buf<double>(h, SC_OUT);   // L: vectors 0 .. d-1, S: 2 .. d+1 at S + k ldv
    hipLaunchKernelGGL(k_ct_chains, dim3(2), dim3(1024), 0, h->stream, d, (const int *)(dm + o_r), (const size_t *)(dm + o_moff), (const double *)buf<double>(h, SC_M), L, S, ldv);
    hipLaunchKernelGGL(k_ct_marg, dim3((unsigned)((pl.wsize + 3) / 4)), dim3(256), 0, h->stream, d, (const CtCore *)(dm + o_cores), (long long)pl.wsize, h->RM, h->P.SS,
                       (const double *)L, (const double *)S, ldv, dout);
    HIPCHECK(hipMemcpyAsync(out, dout, sizeof(double) * pl.wsize, hipMemcpyDeviceToHost, h->stream));
    return ct_finish(h, pl);
}
extern "C" int ttx_contract_modesum(const ttx_engine *h, double *ms, double *bytes)
{
    if (!h || !ms || !bytes) return fail(TTX_EINVAL, "ttx_contract_modesum: null argument");
    *ms = h->ct.ms; *bytes = h->ct.bytes;
    return TTX_OK;
}

// ---- samples from the resident train (ttx_sample.h, ttx_sample_real.h) -----------------------------------------------------------
// What ttx_sample and ttx_sample_real share.  sm_prepare: the plan, the call's tables, the prefix vectors from the effective weights
// (ct_modesum untimed, k_ct_chains), the head tables of the drawn modes (k_sm_head between TM_HEAD's events) and the shape of the draw
// launches.  sm_chunks: the chunk loop with the staging of the host entry, the draw between TM_DRAW's events, the failure count; the squared
// samplers (sq_frame) run their per-mode launches inside it.  The argument checks the four samplers share come first.
namespace {
struct SmLoop { size_t chunk = 0; int gridmax = 0; long long *dcnt = nullptr; };   // what sm_chunks needs: the chunk, the cap of a draw's grid, the failure counter (SC_CNT)
struct SmPrep {                             // what sm_prepare leaves for the chunk loop and the draw launches: outputs only
    SmLoop loop;
    EvTrain T;
    std::vector<size_t> hoff;               // where the head table of a drawn mode starts in SC_H
    std::vector<SmTile> tiles;
    size_t hsize = 0;
    int nrow = 0;                           // the longest drawn mode
    double bytes = 0.0;                     // of the cores k_sm_head reads
    char *dm = nullptr;                     // the call's tables on the device (SC_META)
    size_t o_hoff = 0;
    double *H = nullptr, *grow = nullptr;
    size_t growlen = 0, lds = 0;
    int ldsrow = 0;
};
struct SmStage { void *user; size_t bytes; int slot; void *dev; };    // an output: the caller's array (may be null), bytes per sample, its staging slot; dev: where the chunk's part lies
}
// fixed of ttx_sample and ttx_sample_sq (may be null): 0 for a drawn mode, or the 1-based index a mode is held at
static int sm_check_fixed(const ttx_engine *h, const char *who, const int32_t *fixed)
{
    if (fixed) for (int k = 0; k < h->d; k++) if (fixed[k] < 0 || fixed[k] > h->n1[k + 1]) return fail(TTX_EINVAL, "%s: fixed(%d) = %d (0 .. %d expected)", who, k + 1, fixed[k], h->n1[k + 1]);
    return TTX_OK;
}
// nodes (may be null with npts = 0) and cond (may be null) of the real samplers
static int bs_check_one(const char *who, int k, const ttx_basis &b, int n);     // the node rows are TTX_BASIS_LINEAR's: one check (below, with ttx_basis_batch)
static int sr_check_nodes_cond(const ttx_engine *h, const char *who, const double *const *nodes, const double *cond)
{
    int rc;
    const int d = h->d;
    if (nodes) {
        for (int k = 0; k < d; k++) {
            ttx_basis b{TTX_BASIS_LINEAR, 0, 0.0, 0.0, nodes[k]};
            if ((rc = bs_check_one(who, k + 1, b, h->n1[k + 1]))) return rc;
        }
    }
    if (cond) for (int k = 0; k < d; k++) if (std::isinf(cond[k])) return fail(TTX_EINVAL, "%s: cond(%d) is infinite (a coordinate, or NaN for a drawn mode, expected)", who, k + 1);
    return TTX_OK;
}
// mode and gamma of the squared samplers
static int sq_check_mode_gamma(const char *who, int32_t mode, double gamma)
{
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    if (!(gamma >= 0.0) || !std::isfinite(gamma)) return fail(TTX_EINVAL, "%s: gamma must be a finite number >= 0 (got %g)", who, gamma);
    return TTX_OK;
}
// the chunk of a call of npts >= 1 samples (TTX_SAMPLE_CHUNK, 2^18 by default); asks the device nothing
static size_t sm_chunk(int64_t npts) { return std::min<size_t>(env_chunk("TTX_SAMPLE_CHUNK", (size_t)1 << 18), (size_t)npts); }
// That chunk and the cap of the grid of a draw: one wave per sample (wave_grid).  dcnt
// stays with the caller, who reserves SC_CNT
static SmLoop sm_loop(ttx_engine *h, int64_t npts)
{
    SmLoop L;
    L.chunk = sm_chunk(npts);
    L.gridmax = wave_grid((long long)L.chunk, dev_ncu(h));
    return L;
}
// Inputs: pl, the caller's plan of all modes (ct_plan); held[k] != 0: mode k gets no head table; eff: the effective weights of all modes
// (pl.wsize numbers); hw_ones: k_sm_head multiplies by 1.0 (a block of ones in the call's tables), not by eff; draw_kernel and wave_extra:
// the draw kernel and the doubles of dynamic LDS one of its waves owns on top of 2 ldx + ldsrow.  extra(meta) appends the caller's own
// tables to the call's image before it is uploaded.  Output: P.
template <class Extra>
static int sm_prepare(ttx_engine *h, const char *who, int64_t npts, const CtPlan &pl, const std::vector<char> &held, const std::vector<double> &eff, bool hw_ones,
                      const void *draw_kernel, size_t wave_extra, Extra extra, SmPrep &P)
{
    int rc;
    const int d = h->d;
    if ((rc = ev_train(h, &P.T))) return rc;
    P.hoff.assign(d, 0);
    for (int k = 0; k < d; k++) {
        const CtCore &c = pl.cores[k];
        if (held[k]) continue;
        P.hoff[k] = P.hsize; P.hsize += (size_t)c.n * c.r1;
        P.nrow = std::max(P.nrow, c.n);
        P.bytes += 8.0 * c.r0 * c.n * c.r1;
        const int ti = sm_tile_rows(c.r0);
        for (int b = 0; b < c.r1; b++) for (int i0 = 0; i0 < c.n; i0 += ti) P.tiles.push_back(SmTile{k, b, i0, std::min(ti, c.n - i0)});
    }
    if (P.tiles.size() > 0x7fffffffull) return fail(TTX_EINVAL, "%s: too many head tiles (%zu)", who, P.tiles.size());
    const int ldv = h->RM;
    OpMeta meta(h->meta_host);
    const size_t o_cores = meta.put(pl.cores), o_tiles = meta.put(pl.tiles), o_r = meta.put(pl.r), o_moff = meta.put(pl.moff), o_sm = meta.put(P.tiles);
    P.o_hoff = meta.put(P.hoff);
    extra(meta);
    const size_t o_ones = hw_ones ? meta.put(std::vector<double>(pl.wsize, 1.0)) : 0;
    if ((rc = meta.upload(h, SC_META, &P.dm)) || (rc = buf_reserve(h, SC_VEC, sizeof(double) * (2 * (size_t)d + 4) * ldv)) ||
        (rc = buf_reserve(h, SC_H, sizeof(double) * std::max<size_t>(P.hsize, 1))) || (rc = buf_reserve(h, SC_CNT, sizeof(long long))) ||
        (rc = ct_modesum(h, pl, eff.data(), (const CtCore *)(P.dm + o_cores), (const CtTile *)(P.dm + o_tiles), nullptr))) return rc;   // untimed: ttx_contract_modesum keeps its own last call
    double *L = buf<double>(h, SC_VEC), *S = L + (size_t)d * ldv;
    P.H = buf<double>(h, SC_H);
    P.loop = sm_loop(h, npts);
    P.loop.dcnt = buf<long long>(h, SC_CNT);
    OpTimer &t_head = h->timer[TM_HEAD];
    hipLaunchKernelGGL(k_ct_chains, dim3(2), dim3(1024), 0, h->stream, d, (const int *)(P.dm + o_r), (const size_t *)(P.dm + o_moff), (const double *)buf<double>(h, SC_M), L, S, ldv);
    HIPCHECK(hipMemsetAsync(P.loop.dcnt, 0, sizeof(long long), h->stream));
    if (!P.tiles.empty()) {
        if ((rc = t_head.start(h->stream))) return rc;
        hipLaunchKernelGGL(k_sm_head, dim3((unsigned)P.tiles.size()), dim3(256), 0, h->stream, (const CtCore *)(P.dm + o_cores), (const SmTile *)(P.dm + o_sm), h->RM, h->P.SS,
                           hw_ones ? (const double *)(P.dm + o_ones) : (const double *)buf<double>(h, SC_W), (const double *)L, ldv, (const size_t *)(P.dm + P.o_hoff), P.H);
        if ((rc = t_head.stop(h->stream))) return rc;
    }
    P.ldsrow = std::min(P.nrow, TTX_SM_LDSROW);
    P.growlen = P.nrow > TTX_SM_LDSROW ? (size_t)P.nrow : 0;
    P.lds = 4 * sizeof(double) * (2 * (size_t)P.T.ldx + wave_extra + P.ldsrow);
    if (P.lds > TTX_LDS_DEVICE) return fail(TTX_EINVAL, "%s: %d modes need %zu bytes of LDS per workgroup (160 KB at most)", who, d, P.lds);
    if ((rc = op_lds_raise(h, draw_kernel, op_lds(P.lds)))) return rc;
    if (P.growlen && (rc = buf_reserve(h, SC_ROW, sizeof(double) * P.growlen * 4 * P.loop.gridmax))) return rc;
    P.grow = P.growlen ? buf<double>(h, SC_ROW) : nullptr;
    return TTX_OK;
}
// draw(c, grid, du): the draw launch of a chunk of c samples whose uniforms lie at du; count(c): the launch that adds its failed samples to
// P.dcnt (P: sm_loop's figures and the counter).  Both find the chunk's outputs in out[.].dev (null for an output the caller did not ask for).  *ms_draw, *nfailed: the call's figures
template <class Draw, class Count>
static int sm_chunks(ttx_engine *h, const SmLoop &P, int64_t npts, const double *u, bool dev, SmStage *out, int nout, Draw draw, Count count, double *ms_draw, int64_t *nfailed)
{
    int rc;
    const int d = h->d;
    OpTimer &t_draw = h->timer[TM_DRAW];
    if (!dev) {
        if ((rc = buf_reserve(h, SC_X, sizeof(double) * P.chunk * d))) return rc;
        for (int t = 0; t < nout; t++) if ((rc = buf_reserve(h, out[t].slot, out[t].bytes * P.chunk))) return rc;
    }
    for (int64_t o = 0; o < npts; o += (int64_t)P.chunk) {
        const size_t c = (size_t)std::min<int64_t>((int64_t)P.chunk, npts - o);
        const double *du = u + (size_t)o * d;
        for (int t = 0; t < nout; t++) out[t].dev = out[t].user ? (char *)out[t].user + out[t].bytes * (size_t)o : nullptr;
        if (!dev) {
            HIPCHECK(hipMemcpyAsync(buf<double>(h, SC_X), du, sizeof(double) * c * d, hipMemcpyHostToDevice, h->stream));
            du = buf<double>(h, SC_X);
            for (int t = 0; t < nout; t++) if (out[t].user) out[t].dev = buf<char>(h, out[t].slot);
        }
        const int grid = (int)std::min<long long>(((long long)c + 3) / 4, (long long)P.gridmax);
        if ((rc = t_draw.start(h->stream))) return rc;
        draw(c, grid, du);
        if ((rc = t_draw.stop(h->stream))) return rc;
        count(c);
        if (!dev)
            for (int t = 0; t < nout; t++)
                if (out[t].user) HIPCHECK(hipMemcpyAsync((char *)out[t].user + out[t].bytes * (size_t)o, out[t].dev, out[t].bytes * c, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        HIPCHECK(hipGetLastError());
        double ms = 0.0;
        if ((rc = t_draw.ms(&ms))) return rc;
        *ms_draw += ms;
    }
    long long nf = 0;
    HIPCHECK(hipMemcpy(&nf, P.dcnt, sizeof(long long), hipMemcpyDeviceToHost));
    *nfailed = nf;
    return TTX_OK;
}
// the last-call figures of ttx_sample and ttx_sample_real (which) as their _last entries hand them out; any pointer may be null
static int sm_last(const ttx_engine *h, const char *who, int which, double *ms_head, double *bytes_head, double *ms_draw, int64_t *nfailed)
{
    if (!h) return fail(TTX_EINVAL, "%s: null engine", who);
    const SampleLast &L = h->smp[which];
    if (ms_head) *ms_head = L.ms_head;
    if (bytes_head) *bytes_head = L.bytes;
    if (ms_draw) *ms_draw = L.ms_draw;
    if (nfailed) *nfailed = L.failed;
    return TTX_OK;
}
// both entries: u, ind, logq, val are host pointers (dev false: staged chunk by chunk) or pointers on the engine's device
static int sm_run(ttx_engine *h, const char *who, int64_t npts, const double *u, const double *w, const int32_t *fixed, int32_t *ind, double *logq, double *val, bool dev)
{
    if (npts < 0 || (npts > 0 && (!u || !ind))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    int rc = check_train_one_process(h, who);
    if (rc) return rc;
    const int d = h->d;
    if ((rc = sm_check_fixed(h, who, fixed))) return rc;
    SampleLast &last = h->smp[SMP_GRID];
    last = SampleLast();
    if (npts == 0) return TTX_OK;
    // the effective weights: a fixed mode has the unit vector of its index
    SmPrep P;
    CtPlan pl;
    ct_plan(h, std::vector<char>(d, 1), pl);
    std::vector<double> eff(pl.wsize, 1.0);
    if (w) memcpy(eff.data(), w, sizeof(double) * pl.wsize);
    std::vector<int> fx(d, 0);
    std::vector<char> held(d, 0);
    for (int k = 0; k < d; k++) {
        const CtCore &c = pl.cores[k];
        if (!fixed || !fixed[k]) continue;
        fx[k] = fixed[k]; held[k] = 1;
        for (int i = 0; i < c.n; i++) eff[c.woff + i] = i == fixed[k] - 1 ? 1.0 : 0.0;
    }
    size_t o_fx = 0;
    if ((rc = sm_prepare(h, who, npts, pl, held, eff, false, reinterpret_cast<const void *>(k_sm_draw), (size_t)d + (((size_t)d + 1) >> 1),
                         [&](OpMeta &meta) { o_fx = meta.put(fx); }, P))) return rc;
    last.bytes = P.bytes;
    SmStage out[3] = {{ind, sizeof(int) * (size_t)d, SC_IND, nullptr}, {logq, sizeof(double), SC_LQ, nullptr}, {val, sizeof(double), SC_OUT, nullptr}};
    rc = sm_chunks(h, P.loop, npts, u, dev, out, 3,
        [&](size_t c, int grid, const double *du) {
            hipLaunchKernelGGL(k_sm_draw, dim3(grid), dim3(256), P.lds, h->stream, P.T, (const size_t *)(P.dm + P.o_hoff), (const int *)(P.dm + o_fx), (const double *)P.H, P.ldsrow,
                               P.grow, P.growlen, (long long)c, du, (int *)out[0].dev, (double *)out[1].dev, (double *)out[2].dev);
        },
        [&](size_t c) { hipLaunchKernelGGL(k_sm_count, dim3(1), dim3(1024), 0, h->stream, (long long)c, d, (const int *)out[0].dev, P.loop.dcnt); },
        &last.ms_draw, &last.failed);
    if (rc) return rc;
    return P.tiles.empty() ? TTX_OK : h->timer[TM_HEAD].ms(&last.ms_head);
}
extern "C" int ttx_sample(ttx_engine *h, int64_t npts, const double *u, const double *w, const int32_t *fixed, int32_t *ind, double *logq, double *val)
{
    return sm_run(h, "ttx_sample", npts, u, w, fixed, ind, logq, val, false);
}
extern "C" int ttx_sample_dev(ttx_engine *h, int64_t npts, const double *u, const double *w, const int32_t *fixed, int32_t *ind, double *logq, double *val)
{
    return sm_run(h, "ttx_sample_dev", npts, u, w, fixed, ind, logq, val, true);
}
extern "C" int ttx_sample_last(const ttx_engine *h, double *ms_head, double *bytes_head, double *ms_draw, int64_t *nfailed)
{
    return sm_last(h, "ttx_sample_last", SMP_GRID, ms_head, bytes_head, ms_draw, nfailed);
}


// ---- real-valued samples from the interpolant of the resident train (ttx_sample_real.h) ------------------------------------------
// both entries: u, x, cell, logq, val are host pointers (dev false: staged chunk by chunk) or pointers on the engine's device
static int sr_run(ttx_engine *h, const char *who, int64_t npts, const double *u, const double *const *nodes, const double *cond, double *x, int32_t *cell, double *logq,
                  double *val, bool dev)
{
    if (npts < 0 || (npts > 0 && (!u || !x || !nodes))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    int rc = check_train_one_process(h, who);
    if (rc) return rc;
    const int d = h->d;
    if ((rc = sr_check_nodes_cond(h, who, nodes, cond))) return rc;
    SampleLast &last = h->smp[SMP_REAL];
    last = SampleLast();
    if (npts == 0) return TTX_OK;
    // the effective weights: trapezoid weights of a drawn mode, the hat row of a held one (a mode of one node is held at its node)
    SmPrep P;
    CtPlan pl;
    ct_plan(h, std::vector<char>(d, 1), pl);
    std::vector<double> eff(pl.wsize, 0.0), tnodes;
    std::vector<char> held(d, 0);
    std::vector<SrMode> modes(d);
    for (int k = 0; k < d; k++) {
        const CtCore &c = pl.cores[k];
        const double *t = nodes[k];
        SrMode &M = modes[k];
        M = SrMode{0, 0, 1.0, 0.0, 0.0, tnodes.size()};
        tnodes.insert(tnodes.end(), t, t + c.n);
        const bool given = cond && cond[k] == cond[k];
        if (!given && c.n > 1) { sr_trapezoid(t, c.n, eff.data() + c.woff); continue; }
        held[k] = 1;
        M = sr_held_mode(t, c.n, given ? cond[k] : t[0], M.noff);
        for (int i = 0; i < c.n; i++) eff[c.woff + i] = ttx_basis_entry(TTX_BASIS_LINEAR, 0, 0.0, 0.0, t, c.n, M.xh, i);
    }
    size_t o_modes = 0, o_nodes = 0;
    if ((rc = sm_prepare(h, who, npts, pl, held, eff, true, reinterpret_cast<const void *>(k_sr_draw), 2 * (size_t)d + (((size_t)d + 1) >> 1),
                         [&](OpMeta &meta) { o_modes = meta.put(modes); o_nodes = meta.put(tnodes); }, P))) return rc;
    last.bytes = P.bytes;
    SmStage out[4] = {{x, sizeof(double) * (size_t)d, SC_SRX, nullptr}, {cell, sizeof(int) * (size_t)d, SC_IND, nullptr}, {logq, sizeof(double), SC_LQ, nullptr},
                      {val, sizeof(double), SC_OUT, nullptr}};
    rc = sm_chunks(h, P.loop, npts, u, dev, out, 4,
        [&](size_t c, int grid, const double *du) {
            hipLaunchKernelGGL(k_sr_draw, dim3(grid), dim3(256), P.lds, h->stream, P.T, (const size_t *)(P.dm + P.o_hoff), (const SrMode *)(P.dm + o_modes),
                               (const double *)(P.dm + o_nodes), (const double *)P.H, P.ldsrow, P.grow, P.growlen, (long long)c, du, (double *)out[0].dev, (int *)out[1].dev,
                               (double *)out[2].dev, (double *)out[3].dev);
        },
        [&](size_t c) { hipLaunchKernelGGL(k_sr_count, dim3(1), dim3(1024), 0, h->stream, (long long)c, d, (const double *)out[0].dev, P.loop.dcnt); },
        &last.ms_draw, &last.failed);
    if (rc) return rc;
    return P.tiles.empty() ? TTX_OK : h->timer[TM_HEAD].ms(&last.ms_head);
}
extern "C" int ttx_sample_real(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double *x, int32_t *cell, double *logq, double *val)
{
    return sr_run(h, "ttx_sample_real", npts, u, nodes, cond, x, cell, logq, val, false);
}
extern "C" int ttx_sample_real_dev(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double *x, int32_t *cell, double *logq, double *val)
{
    return sr_run(h, "ttx_sample_real_dev", npts, u, nodes, cond, x, cell, logq, val, true);
}
extern "C" int ttx_sample_real_last(const ttx_engine *h, double *ms_head, double *bytes_head, double *ms_draw, int64_t *nfailed)
{
    return sm_last(h, "ttx_sample_real_last", SMP_REAL, ms_head, bytes_head, ms_draw, nfailed);
}

// ---- sums and elementwise products of resident trains (ttx_algebra.h) -----------------------------------------------------------
static bool alg_even16(const void *p, int RM, size_t SS) { return ((uintptr_t)p & 15) == 0 && RM % 2 == 0 && SS % 2 == 0; }
static int alg_ta(int rows, int vec)
{
    const int need = vec ? (rows + 1) / 2 : rows;
    int ta = 1;
    while (ta < 64 && ta < need) ta <<= 1;
    return ta;
}
// what both operations ask of their operands, before any device call: every engine holds a train (one that spreads it over
// processes gets ttx_ijk's answer), same modes, same device, boundary ranks 1
static int alg_check(const char *who, int m, ttx_engine *const *x)
{
    for (int t = 0; t < m; t++) if (!x[t]) return fail(TTX_EINVAL, "%s: null engine (operand %d)", who, t + 1);
    for (int t = 0; t < m; t++) {
        if (!x[t]->ran) return fail(TTX_ESTATE, "%s: no tensor train in operand %d (run dtt_dmrgg first)", who, t + 1);
        if (x[t]->W > 1) return tt_prepare(x[t], who);
    }
    const ttx_engine *h = x[0];
    for (int t = 0; t < m; t++) {
        if (x[t]->d != h->d) return fail(TTX_EINVAL, "%s: dimensions not match (operand %d has %d modes, operand 1 %d)", who, t + 1, x[t]->d, h->d);
        for (int k = 1; k <= h->d; k++) if (x[t]->n1[k] != h->n1[k]) return fail(TTX_EINVAL, "%s: sizes not match (mode %d: operand %d has %d, operand 1 %d)", who, k, t + 1, x[t]->n1[k], h->n1[k]);
        if (x[t]->cfg.device != h->cfg.device) return fail(TTX_EINVAL, "%s: all tensor trains must live on the same GPU", who);
        if (x[t]->rfinal[0] != 1 || x[t]->rfinal[h->d] != 1) return fail(TTX_EINVAL, "%s: boundary ranks of operand %d are not 1", who, t + 1);
    }
    return TTX_OK;
}
// the block table to the device, the one launch between the timer's events, the wait
static int alg_launch(ttx_engine *h, ttx_engine *e, const std::vector<AlgBlk> &blks, long long tiles, bool hadamard, double rd, double wr)
{
    int rc;
    OpMeta meta(h->meta_host);
    meta.put(blks);
    char *dm;
    if ((rc = meta.upload(h, SC_META, &dm))) return rc;
    OpTimer &tm = h->timer[TM_ALG];
    h->alg = AlgLast{0.0, rd, wr};
    if ((rc = tm.start(h->stream))) return rc;
    if (hadamard) hipLaunchKernelGGL(k_alg_hadamard, dim3((unsigned)tiles), dim3(256), 0, h->stream, (const AlgBlk *)dm, (int)blks.size(), e->RM, e->P.SS);
    else hipLaunchKernelGGL(k_alg_lincomb, dim3((unsigned)tiles), dim3(256), 0, h->stream, (const AlgBlk *)dm, (int)blks.size(), e->RM, e->P.SS);
    if ((rc = tm.stop(h->stream))) return rc;
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return tm.ms(&h->alg.ms);
}
static int alg_lincomb_fill(int m, const double *coef, ttx_engine *const *x, ttx_engine *e)
{
    ttx_engine *h = x[0];
    const int d = h->d;
    std::vector<AlgBlk> blks;
    blks.reserve((size_t)d * m);
    long long tiles = 0;
    double rd = 0.0, wr = 0.0;
    for (int k = 0; k < d; k++) {
        const int n = h->n1[k + 1], R0 = e->rfinal[k];
        wr += 8.0 * R0 * n * e->rfinal[k + 1];
        int ro = 0, co = 0;
        for (int t = 0; t < m; t++) {
            AlgBlk B{};
            B.x = core_dev(x[t], k + 1); B.xRM = x[t]->RM; B.xSS = x[t]->P.SS;
            B.dst = core_dev(e, k + 1) + e->P.SS * (size_t)co;
            B.coef = coef[t]; B.scale = k == 0; B.fill = k < d - 1;
            B.R0 = R0; B.ro = ro; B.r0 = x[t]->rfinal[k]; B.n = n; B.r1 = x[t]->rfinal[k + 1];
            B.vec = alg_even16(B.x, B.xRM, B.xSS) && alg_even16(B.dst, e->RM, e->P.SS) && ro % 2 == 0;
            B.ta = alg_ta(B.fill ? R0 : B.r0, B.vec);
            B.first = tiles;
            const long long per = (long long)(256 / B.ta) * TTX_ALG_U;
            tiles += ((long long)n * B.r1 + per - 1) / per;
            rd += 8.0 * B.r0 * n * B.r1;
            blks.push_back(B);
            if (k > 0) ro += B.r0;
            if (k < d - 1) co += B.r1;
        }
    }
    if (tiles > 0x7fffffffll) return fail(TTX_EINVAL, "ttx_lincomb: too many tiles (%lld)", tiles);
    return alg_launch(h, e, blks, tiles, false, rd, wr);
}
extern "C" int ttx_lincomb(int32_t m, const double *coef, ttx_engine *const *x, ttx_engine **out)
{
    if (out) *out = nullptr;
    if (!coef || !x || !out) return fail(TTX_EINVAL, "ttx_lincomb: null argument");
    if (m < 1) return fail(TTX_EINVAL, "ttx_lincomb: %d terms (at least one expected)", m);
    int rc = alg_check("ttx_lincomb", m, x);
    if (rc) return rc;
    ttx_engine *h = x[0];
    const int d = h->d;
    std::vector<int32_t> nn = modes_of(h), rr(d + 1, 1);
    for (int k = 1; k < d; k++) {
        long long s = 0;
        for (int t = 0; t < m; t++) s += x[t]->rfinal[k];
        if (s > 128) return fail(TTX_EINVAL, "ttx_lincomb: the ranks at bond %d add up to %lld, the engine holds ranks up to 128 (round the terms first: ttx_svd)", k, s);
        rr[k] = (int32_t)s;
    }
    HIPCHECK(hipSetDevice(h->cfg.device));
    return new_train(out, "ttx_lincomb", d, nn.data(), rr.data(), h->cfg.device, [&](ttx_engine *e) { return alg_lincomb_fill(m, coef, x, e); });
}
static int alg_hadamard_fill(ttx_engine *x, ttx_engine *y, ttx_engine *e)
{
    const int d = x->d;
    std::vector<AlgBlk> blks(d);
    long long tiles = 0;
    double rd = 0.0, wr = 0.0;
    for (int k = 0; k < d; k++) {
        AlgBlk &B = blks[k];
        B = AlgBlk{};
        B.x = core_dev(x, k + 1); B.xRM = x->RM; B.xSS = x->P.SS;
        B.y = core_dev(y, k + 1); B.yRM = y->RM; B.ySS = y->P.SS;
        B.dst = core_dev(e, k + 1);
        B.n = x->n1[k + 1]; B.r0 = x->rfinal[k]; B.r1 = x->rfinal[k + 1]; B.ry0 = y->rfinal[k]; B.ry1 = y->rfinal[k + 1];
        B.R0 = B.r0 * B.ry0;
        B.vec = B.r0 % 2 == 0 && alg_even16(B.x, B.xRM, B.xSS) && alg_even16(B.dst, e->RM, e->P.SS);
        B.ta = alg_ta(B.R0, B.vec);
        B.ntk = (B.r1 + TTX_ALG_KC - 1) / TTX_ALG_KC;
        B.first = tiles;
        const long long cpw = 256 / B.ta;
        tiles += (((long long)B.n * B.ry1 + cpw - 1) / cpw) * B.ntk;
        rd += 8.0 * B.n * ((double)B.r0 * B.r1 + (double)B.ry0 * B.ry1);
        wr += 8.0 * B.R0 * B.n * ((double)B.r1 * B.ry1);
    }
    if (tiles > 0x7fffffffll) return fail(TTX_EINVAL, "ttx_hadamard: too many tiles (%lld)", tiles);
    return alg_launch(x, e, blks, tiles, true, rd, wr);
}
extern "C" int ttx_hadamard(ttx_engine *x, ttx_engine *y, ttx_engine **out)
{
    if (out) *out = nullptr;
    if (!x || !y || !out) return fail(TTX_EINVAL, "ttx_hadamard: null argument");
    ttx_engine *const xy[2] = {x, y};
    int rc = alg_check("ttx_hadamard", 2, xy);
    if (rc) return rc;
    const int d = x->d;
    std::vector<int32_t> nn = modes_of(x), rr(d + 1, 1);
    for (int k = 1; k < d; k++) {
        const int p = x->rfinal[k] * y->rfinal[k];
        if (p > 128) return fail(TTX_EINVAL, "ttx_hadamard: the ranks at bond %d multiply to %d (%d x %d), the engine holds ranks up to 128 (round the factors first: ttx_svd)", k, p, x->rfinal[k], y->rfinal[k]);
        rr[k] = p;
    }
    HIPCHECK(hipSetDevice(x->cfg.device));
    return new_train(out, "ttx_hadamard", d, nn.data(), rr.data(), x->cfg.device, [&](ttx_engine *e) { return alg_hadamard_fill(x, y, e); });
}
extern "C" int ttx_algebra_last(const ttx_engine *h, double *ms, double *bytes_read, double *bytes_written)
{
    if (!h || !ms || !bytes_read || !bytes_written) return fail(TTX_EINVAL, "ttx_algebra_last: null argument");
    *ms = h->alg.ms; *bytes_read = h->alg.rd; *bytes_written = h->alg.wr;
    return TTX_OK;
}

// ---- a rounded sum of resident trains (ttx_roundsum.h) ----------------------------------------------------------------------------
// everything of ttx_lincomb_round that works on the new engine e (ranks l): a failure leaves e to the caller to destroy.  All launches go
// to x[0]'s stream: e runs on it for the length of the call (qr(), unpack_core and svd_impl launch on their engine's stream).
static int rs_fill(int m, const double *coef, ttx_engine *const *x, ttx_engine *e, const std::vector<long long> &S, const int32_t *l, double tol, int rmax,
                   unsigned long long seed, int mode)
{
    ttx_engine *h = x[0];
    const int d = h->d;
    int rc;
    if ((rc = tt_prepare(e, "ttx_lincomb_round"))) return rc;
    struct OnStream { ttx_engine *e; hipStream_t own; ~OnStream() { e->stream = own; } } on{e, e->stream};
    e->stream = h->stream;
    std::vector<const int32_t *> rt(m);
    for (int t = 0; t < m; t++) rt[t] = x[t]->rfinal.data();
    RsPlan pl = rs_plan(d, h->n1.data() + 1, m, rt.data(), S.data(), l, mode);
    if (pl.refused) return fail(TTX_EINVAL, "ttx_lincomb_round: too many tiles (%lld)", pl.refused);
    for (int k = 1; k <= d; k++)
        for (int t = 0; t < m; t++) { RsBlk &B = pl.blks[(size_t)(k - 1) * m + t]; B.x = core_dev(x[t], k); B.RM = x[t]->RM; B.SS = x[t]->P.SS; }
    const std::vector<RsBlk> &blks = pl.blks;
    const std::vector<size_t> &ooff = pl.ooff, &woff = pl.woff;
    const std::vector<long long> &tS = pl.tS, &tA = pl.tA;
    const int eff = pl.eff;
    h->rs = RsLast();
    h->rs.flops = pl.fl; h->rs.mode = eff; h->rs.l.assign(l, l + d + 1);
    OpMeta meta(h->meta_host);
    const size_t o_blk = meta.put(blks), o_off = meta.put(ooff);
    char *dm;
    if ((rc = meta.upload(h, SC_RSTAB, &dm)) || (rc = buf_reserve(h, SC_RSO, sizeof(double) * std::max<size_t>(ooff[d], 1))) ||
        (rc = buf_reserve(h, SC_RSW, sizeof(double) * woff[d + 1])) || (rc = buf_reserve(h, SC_RSYA, sizeof(double) * pl.ymax)) ||
        (rc = buf_reserve(h, SC_RSYB, sizeof(double) * pl.ymax)) || (rc = buf_reserve(h, SC_RSM, sizeof(double) * pl.mmax))) return rc;
    const RsBlk *dblk = (const RsBlk *)(dm + o_blk);
    double *Om = buf<double>(h, SC_RSO), *W = buf<double>(h, SC_RSW), *Y = buf<double>(h, SC_RSYA), *Yn = buf<double>(h, SC_RSYB), *M = buf<double>(h, SC_RSM);
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(k_rs_omega, dim3(g1(pl.omax).x, d), dim3(256), 0, st, seed, (const size_t *)(dm + o_off), Om);
    // right to left: W(d) = ones, W(k-1) from W(k)
    OpTimer &tm = h->timer[TM_RS_SKETCH];
    if ((rc = tm.start(st))) return rc;
    hipLaunchKernelGGL(k_fill_const, g1((size_t)m), dim3(256), 0, st, (size_t)m, W + woff[d], 1.0);
    for (int k = d; k >= 2; k--) {
        const int n = h->n1[k], l0 = l[k - 1], l1 = l[k];
        if (eff == TTX_EVAL_MFMA)
            hipLaunchKernelGGL(k_rs_sketch<true>, dim3((unsigned)tS[k]), dim3(256), 0, st, dblk + (size_t)(k - 1) * m, m, n, l0, l1, (const double *)(Om + ooff[k - 1]),
                               (const double *)(W + woff[k]), (int)S[k], W + woff[k - 1], (int)S[k - 1]);
        else
            hipLaunchKernelGGL(k_rs_sketch<false>, dim3((unsigned)tS[k]), dim3(256), 0, st, dblk + (size_t)(k - 1) * m, m, n, l0, l1, (const double *)(Om + ooff[k - 1]),
                               (const double *)(W + woff[k]), (int)S[k], W + woff[k - 1], (int)S[k - 1]);
        hipLaunchKernelGGL(k_rs_scale, dim3(1), dim3(1024), 0, st, (size_t)S[k - 1] * l0, W + woff[k - 1]);
    }
    if ((rc = tm.stop(st))) return rc;
    // left to right
    const TtScratch s(e);
    OpMarks marks(h->op_ev);                // phases 1 gemm, 2 qr, 3 advance; 0 is the sketch's (TM_RS_SKETCH)
    HIPCHECK(hipMemcpyAsync(M, coef, sizeof(double) * m, hipMemcpyHostToDevice, st));
    if ((rc = marks.mark(st, 0))) return rc;
    auto advance = [&](int k, int lr, int ldm, double *dst) {                   // Y(k) from M (lr rows) and the cores k
        const int n = h->n1[k];
        if (eff == TTX_EVAL_MFMA)
            hipLaunchKernelGGL(k_rs_advance<true>, dim3((unsigned)tA[k]), dim3(256), 0, st, dblk + (size_t)(k - 1) * m, m, n, lr, (lr + 15) / 16, (const double *)M, ldm, dst, (size_t)lr * n);
        else
            hipLaunchKernelGGL(k_rs_advance<false>, dim3((unsigned)tA[k]), dim3(256), 0, st, dblk + (size_t)(k - 1) * m, m, n, lr, (lr + 15) / 16, (const double *)M, ldm, dst, (size_t)lr * n);
        return marks.mark(st, 3);
    };
    if ((rc = advance(1, 1, 1, Y))) return rc;
    for (int k = 1; k < d; k++) {
        const int rows = l[k - 1] * h->n1[k], l1 = l[k], Sk = (int)S[k];
        gemm(e, rows, l1, Sk, Y, rows, W + woff[k], Sk, e->Wa, rows);                       // Z = Y(k) W(k)
        if ((rc = marks.mark(st, 1)) || (rc = qr(e, rows, l1, e->Wa, s.Rm, s.tau))) return rc;
        unpack_core(e, k, e->Wa, l[k - 1], l1);                                             // new core k = Q
        hipLaunchKernelGGL(k_transpose, g1((size_t)rows * l1), dim3(256), 0, st, rows, l1, (const double *)e->Wa, e->Wb);
        if ((rc = marks.mark(st, 2))) return rc;
        gemm(e, l1, Sk, rows, e->Wb, l1, Y, rows, M, l1);                                   // M = Q^T Y(k)
        if ((rc = marks.mark(st, 1)) || (rc = advance(k + 1, l1, l1, Yn))) return rc;
        std::swap(Y, Yn);
    }
    const int lr = l[d - 1], nd = h->n1[d];
    hipLaunchKernelGGL(k_rs_last, g1((size_t)lr * nd), dim3(256), 0, st, lr, nd, m, (const double *)Y, (size_t)lr * nd, core_dev(e, d), e->RM);
    if ((rc = marks.mark(st, 3))) return rc;
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipGetLastError());
    if ((rc = tm.ms(&h->rs.ms[0])) || (rc = marks.sum(h->rs.ms))) return rc;
    if (tol >= 0.0 && (rc = svd_impl(e, tol, rmax))) return rc;
    HIPCHECK(hipStreamSynchronize(st));
    return TTX_OK;
}
extern "C" int ttx_lincomb_round(int32_t m, const double *coef, ttx_engine *const *x, int32_t rsketch, double tol, int32_t rmax, uint64_t seed, int32_t mode,
                                 ttx_engine **out)
{
    if (out) *out = nullptr;
    if (!coef || !x || !out) return fail(TTX_EINVAL, "ttx_lincomb_round: null argument");
    if (m < 1) return fail(TTX_EINVAL, "ttx_lincomb_round: %d terms (at least one expected)", m);
    if (m > TTX_RS_MAXTERMS) return fail(TTX_EINVAL, "ttx_lincomb_round: %d terms, at most %d are taken", m, TTX_RS_MAXTERMS);
    if (rsketch < 0 || rsketch > 128) return fail(TTX_EINVAL, "ttx_lincomb_round: sketch rank %d (0 = 128, or 1 .. 128: the engine holds ranks up to 128)", rsketch);
    if (rmax < 0) return fail(TTX_EINVAL, "ttx_lincomb_round: rmax must be >= 0 (0: absent; got %d)", (int)rmax);
    if (tol != tol) return fail(TTX_EINVAL, "ttx_lincomb_round: tol is not a number (tol < 0 skips the truncation)");
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "ttx_lincomb_round: unknown mode %d", mode);
    int rc = alg_check("ttx_lincomb_round", m, x);
    if (rc) return rc;
    ttx_engine *h = x[0];
    const int d = h->d;
    std::vector<int32_t> nn = modes_of(h), ll(d + 1, 1);
    std::vector<long long> S(d + 1, m);
    for (int k = 1; k < d; k++) {
        S[k] = 0;
        for (int t = 0; t < m; t++) S[k] += x[t]->rfinal[k];
        if (S[k] > TTX_RS_MAXSUM) return fail(TTX_EINVAL, "ttx_lincomb_round: the ranks at bond %d add up to %lld, at most %d are taken", k, S[k], TTX_RS_MAXSUM);
    }
    rs_sketch_ranks(d, nn.data(), S.data(), rsketch ? rsketch : 128, ll.data());
    HIPCHECK(hipSetDevice(h->cfg.device));
    return new_train(out, "ttx_lincomb_round", d, nn.data(), ll.data(), h->cfg.device,
                     [&](ttx_engine *e) { return rs_fill(m, coef, x, e, S, ll.data(), tol, rmax, (unsigned long long)seed, mode); });
}
extern "C" int ttx_roundsum_last(const ttx_engine *h, double *ms, double *flops, int32_t *lsk, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_roundsum_last: null engine");
    if (ms) for (int p = 0; p < 4; p++) ms[p] = h->rs.ms[p];
    if (flops) *flops = h->rs.flops;
    if (lsk) for (int k = 0; k <= h->d; k++) lsk[k] = k < (int)h->rs.l.size() ? h->rs.l[k] : 0;
    if (mode_ran) *mode_ran = h->rs.mode;
    return TTX_OK;
}

// ---- matrices applied to chosen modes (ttx_modeapply.h) -------------------------------------------------------------------------
// everything of ttx_mode_apply that works on the new engine e: a failure leaves e to the caller to destroy
static int ma_fill(ttx_engine *h, ttx_engine *e, const int32_t *m, const double *A, bool dev, int mode)
{
    MaPlan pl = ma_plan(h->d, h->n1.data() + 1, h->rfinal.data(), m, mode);
    if (pl.refused) return fail(TTX_EINVAL, "ttx_mode_apply: too many tiles (%lld)", std::max(pl.tapp, pl.tcpy));
    std::vector<MaCore> &app = pl.app, &cpy = pl.cpy;
    const long long tapp = pl.tapp, tcpy = pl.tcpy;
    int rc;
    const double *dA = A;
    if (!dev && pl.asize) {
        if ((rc = buf_reserve(h, SC_MAT, sizeof(double) * pl.asize))) return rc;
        HIPCHECK(hipMemcpyAsync(buf<double>(h, SC_MAT), A, sizeof(double) * pl.asize, hipMemcpyHostToDevice, h->stream));
        dA = buf<double>(h, SC_MAT);
    }
    for (size_t t = 0; t < app.size(); t++) { app[t].src = core_dev(h, pl.app_k[t] + 1); app[t].dst = core_dev(e, pl.app_k[t] + 1); app[t].A = dA + pl.aoff[t]; }
    for (size_t t = 0; t < cpy.size(); t++) { cpy[t].src = core_dev(h, pl.cpy_k[t] + 1); cpy[t].dst = core_dev(e, pl.cpy_k[t] + 1); }
    OpMeta meta(h->meta_host);
    const size_t o_app = meta.put(app), o_cpy = meta.put(cpy);
    char *dm;
    if ((rc = meta.upload(h, SC_META, &dm))) return rc;
    h->ma = MaLast{0.0, pl.rd, pl.wr, pl.fl, pl.eff};
    if (!cpy.empty())
        hipLaunchKernelGGL(k_ma_copy, dim3((unsigned)tcpy), dim3(256), 0, h->stream, (const MaCore *)(dm + o_cpy), (int)cpy.size(), h->RM, h->P.SS, e->RM, e->P.SS);
    OpTimer &tm = h->timer[TM_APPLY];
    if (!app.empty()) {
        if ((rc = tm.start(h->stream))) return rc;
        if (pl.eff == TTX_EVAL_MFMA)
            hipLaunchKernelGGL(k_ma_apply<true>, dim3((unsigned)tapp), dim3(256), 0, h->stream, (const MaCore *)(dm + o_app), (int)app.size(), h->RM, h->P.SS, e->RM, e->P.SS);
        else
            hipLaunchKernelGGL(k_ma_apply<false>, dim3((unsigned)tapp), dim3(256), 0, h->stream, (const MaCore *)(dm + o_app), (int)app.size(), h->RM, h->P.SS, e->RM, e->P.SS);
        if ((rc = tm.stop(h->stream))) return rc;
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return app.empty() ? TTX_OK : tm.ms(&h->ma.ms);
}
static int ma_run(ttx_engine *h, const int32_t *m, const double *A, int32_t mode, ttx_engine **out, bool dev, const char *who)
{
    if (out) *out = nullptr;
    if (!h || !m || !out) return fail(TTX_EINVAL, "%s: null argument", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    const int d = h->d;
    bool any = false;
    for (int k = 0; k < d; k++) {
        if (m[k] < 0) return fail(TTX_EINVAL, "%s: m(%d) = %d (0 = the mode is left alone, or a positive size)", who, k + 1, m[k]);
        any = any || m[k] > 0;
    }
    if (any && !A) return fail(TTX_EINVAL, "%s: null matrices", who);
    if (!h->ran) return fail(TTX_ESTATE, "%s: no tensor train (run dtt_dmrgg first)", who);
    const int rmax = std::max(1, (int)*std::max_element(h->rfinal.begin(), h->rfinal.begin() + d + 1));
    std::vector<int32_t> nn = modes_of(h), rr(h->rfinal.begin(), h->rfinal.begin() + d + 1);
    for (int k = 0; k < d; k++) {
        if (m[k] == 0) continue;
        if (m[k] > 32000) return fail(TTX_EINVAL, "%s: m(%d) = %d, the engine holds modes up to 32000", who, k + 1, m[k]);
        if ((long long)rmax * m[k] > (long long)TTX_MAXPART * TTX_BLK)
            return fail(TTX_EINVAL, "%s: m(%d) = %d times the largest rank %d is %lld, the engine holds up to %d", who, k + 1, m[k], rmax, (long long)rmax * m[k], TTX_MAXPART * TTX_BLK);
        nn[k] = m[k];
    }
    if (int rc = check_train_one_process(h, who)) return rc;
    return new_train(out, who, d, nn.data(), rr.data(), h->cfg.device, [&](ttx_engine *e) { return ma_fill(h, e, m, A, dev, mode); });
}
extern "C" int ttx_mode_apply(ttx_engine *h, const int32_t *m, const double *A, int32_t mode, ttx_engine **out)
{
    return ma_run(h, m, A, mode, out, false, "ttx_mode_apply");
}
extern "C" int ttx_mode_apply_dev(ttx_engine *h, const int32_t *m, const double *A_dev, int32_t mode, ttx_engine **out)
{
    return ma_run(h, m, A_dev, mode, out, true, "ttx_mode_apply_dev");
}
extern "C" int ttx_mode_apply_last(const ttx_engine *h, double *ms, double *bytes_read, double *bytes_written, double *flops, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_mode_apply_last: null engine");
    if (ms) *ms = h->ma.ms;
    if (bytes_read) *bytes_read = h->ma.rd;
    if (bytes_written) *bytes_written = h->ma.wr;
    if (flops) *flops = h->ma.flops;
    if (mode_ran) *mode_ran = h->ma.mode;
    return TTX_OK;
}

// ---- the train in a function basis at real points (ttx_basis.h) ------------------------------------------------------------------
// one mode's descriptor as the header states it: a known kind, a < b both finite, n finite strictly ascending nodes
static int bs_check_one(const char *who, int k, const ttx_basis &b, int n)
{
    if (b.kind == TTX_BASIS_COS) {
        if (!std::isfinite(b.a) || !std::isfinite(b.b) || !(b.a < b.b)) return fail(TTX_EINVAL, "%s: mode %d: a finite interval a < b expected (got %g, %g)", who, k, b.a, b.b);
        return TTX_OK;
    }
    if (b.kind != TTX_BASIS_LINEAR) return fail(TTX_EINVAL, "%s: mode %d: unknown basis kind %d", who, k, b.kind);
    if (!b.nodes) return fail(TTX_EINVAL, "%s: mode %d: TTX_BASIS_LINEAR without nodes", who, k);
    for (int j = 0; j < n; j++) {
        if (!std::isfinite(b.nodes[j])) return fail(TTX_EINVAL, "%s: mode %d: node %d is not finite", who, k, j);
        if (j && !(b.nodes[j - 1] < b.nodes[j])) return fail(TTX_EINVAL, "%s: mode %d: the nodes are not strictly ascending at %d", who, k, j);
    }
    return TTX_OK;
}
extern "C" int ttx_basis_host(const ttx_basis *b, int32_t n, int64_t npts, const double *x, int64_t ldx, double *phi)
{
    const char *who = "ttx_basis_host";
    if (!b || n < 1 || npts < 0 || ldx < 1 || (npts > 0 && (!x || !phi))) return fail(TTX_EINVAL, "%s: null argument, n < 1, npts < 0 or ldx < 1", who);
    if (int rc = bs_check_one(who, 1, *b, n)) return rc;
    const double w = b->kind == TTX_BASIS_COS ? ttx_basis_cos_w(b->a, b->b) : 0.0;
    for (int64_t p = 0; p < npts; p++)
        for (int j = 0; j < n; j++) phi[(size_t)p * n + j] = ttx_basis_entry(b->kind, b->flags, b->a, w, b->nodes, n, x[(size_t)p * ldx], j);
    return TTX_OK;
}
enum { BSM_TABLE, BSM_CHAIN };             // OpMarks phases of a call: every launch is followed by the mark of its kind, BsLast::ms takes the sums
static int bs_run(ttx_engine *h, const char *who, BsSrc src, int64_t npts, const double *in, const ttx_basis *basis, double *out, int32_t mode)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (npts < 0 || (npts > 0 && (!in || !out || (!tab && !basis)))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    const int d = h->d;
    if (!tab && basis) for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    const BsPlan pl = bs_plan(d, h->n1.data() + 1, h->rfinal.data(), dev_ncu(h), src, npts, mode, env_chunk("TTX_BASIS_CHUNK", op_chunk_default(h->RM)));
    if (pl.refusal == BS_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.rmax);
    if (pl.refusal == BS_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    h->bs = BsLast();
    h->bs.flops = pl.flops; h->bs.mode = pl.eff;
    if (npts == 0) return TTX_OK;
    EvTrain T;
    if ((rc = ev_train(h, &T))) return rc;
    // the nodes of the LINEAR modes, one device block
    std::vector<BsMode> M(d);
    if (!tab) {
        OpMeta meta(h->meta_host);
        std::vector<size_t> o_nodes(d, 0);
        for (int k = 0; k < d; k++)
            if (basis[k].kind == TTX_BASIS_LINEAR) o_nodes[k] = meta.put(std::vector<double>(basis[k].nodes, basis[k].nodes + h->n1[k + 1]));
        char *dm = nullptr;
        if (!meta.host.empty() && (rc = meta.upload(h, SC_META, &dm))) return rc;
        for (int k = 0; k < d; k++) {
            const ttx_basis &b = basis[k];
            const bool cosk = b.kind == TTX_BASIS_COS;
            M[k] = BsMode{b.kind, b.flags, h->n1[k + 1], cosk ? b.a : 0.0, cosk ? ttx_basis_cos_w(b.a, b.b) : 0.0, cosk ? nullptr : (const double *)(dm + o_nodes[k])};
        }
    }
    if ((rc = buf_reserve(h, {{SC_XA, pl.b_xa}, {SC_XB, pl.b_xb}, {SC_BTAB, pl.b_btab}, {SC_X, pl.b_x}, {SC_OUT, pl.b_out}}))) return rc;
    double *btab = buf<double>(h, SC_BTAB), *sin_ = buf<double>(h, SC_X), *sout = buf<double>(h, SC_OUT);
    OpMarks marks(h->op_ev);
    for (int64_t o = 0; o < npts; o += (int64_t)pl.chunk) {
        const int c = (int)std::min<int64_t>((int64_t)pl.chunk, npts - o);
        const double *cin = in + (size_t)o * pl.row;
        double *cout = out + o;
        if (!dev) {
            HIPCHECK(hipMemcpyAsync(sin_, cin, sizeof(double) * (size_t)c * pl.row, hipMemcpyHostToDevice, h->stream));
            cin = sin_; cout = sout;
        }
        double *X = buf<double>(h, SC_XA), *Z = buf<double>(h, SC_XB);
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        for (int i = d - 1; i >= 0; i--) {
            const double *ph = cin + pl.off[i];
            size_t ld = pl.sumn;
            if (!tab) {
                hipLaunchKernelGGL(k_bs_table, g1((size_t)c * M[i].n), dim3(256), 0, h->stream, M[i], (long long)c, cin + i, d, btab);
                if ((rc = marks.mark(h->stream, BSM_TABLE))) return rc;
                ph = btab; ld = (size_t)M[i].n;
            }
            const double *Xin = i == d - 1 ? nullptr : X;
            double *o1 = i == 0 ? cout : nullptr;
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bs_exact, dim3(pl.g_exact(c)), dim3(256), pl.exact_lds, h->stream, T, i, (long long)c, ph, ld, Xin, Z, o1);
            else
                with_tier<true>(pl.step[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL(k_bs_gemm<decltype(mr)::value>, dim3(pl.g_gemm(i, c)), dim3(256), pl.step[i].lds, h->stream, T, i, c, ph, ld, Xin, Z, o1);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, BSM_CHAIN))) return rc;
            std::swap(X, Z);
        }
        if (!dev) HIPCHECK(hipMemcpyAsync(out + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
        if (!dev || marks.phase.size() > 4096) {                                // the staging blocks are reused by the next chunk; the event chain stays short
            HIPCHECK(hipStreamSynchronize(h->stream));
            if ((rc = marks.sum(h->bs.ms))) return rc;
        }
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = marks.sum(h->bs.ms))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_basis_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, double *out, int32_t mode)
{
    return bs_run(h, "ttx_basis_batch", BS_X_HOST, npts, x, basis, out, mode);
}
extern "C" int ttx_basis_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, double *out_dev, int32_t mode)
{
    return bs_run(h, "ttx_basis_batch_dev", BS_X_DEV, npts, x_dev, basis, out_dev, mode);
}
extern "C" int ttx_basis_tab(ttx_engine *h, int64_t npts, const double *phi, double *out, int32_t mode)
{
    return bs_run(h, "ttx_basis_tab", BS_TAB_HOST, npts, phi, nullptr, out, mode);
}
extern "C" int ttx_basis_tab_dev(ttx_engine *h, int64_t npts, const double *phi_dev, double *out_dev, int32_t mode)
{
    return bs_run(h, "ttx_basis_tab_dev", BS_TAB_DEV, npts, phi_dev, nullptr, out_dev, mode);
}
extern "C" int ttx_basis_last(const ttx_engine *h, double *ms_table, double *ms_chain, double *flops, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_basis_last: null engine");
    if (ms_table) *ms_table = h->bs.ms[BSM_TABLE];
    if (ms_chain) *ms_chain = h->bs.ms[BSM_CHAIN];
    if (flops) *flops = h->bs.flops;
    if (mode_ran) *mode_ran = h->bs.mode;
    return TTX_OK;
}

// ---- value and gradient of the train in a function basis (ttx_basis_grad.h) ------------------------------------------------------
extern "C" int ttx_basis_host_d(const ttx_basis *b, int32_t n, int64_t npts, const double *x, int64_t ldx, double *dphi)
{
    const char *who = "ttx_basis_host_d";
    if (!b || n < 1 || npts < 0 || ldx < 1 || (npts > 0 && (!x || !dphi))) return fail(TTX_EINVAL, "%s: null argument, n < 1, npts < 0 or ldx < 1", who);
    if (int rc = bs_check_one(who, 1, *b, n)) return rc;
    const double w = b->kind == TTX_BASIS_COS ? ttx_basis_cos_w(b->a, b->b) : 0.0;
    for (int64_t p = 0; p < npts; p++)
        for (int j = 0; j < n; j++) dphi[(size_t)p * n + j] = ttx_basis_dentry(b->kind, b->flags, b->a, w, b->nodes, n, x[(size_t)p * ldx], j);
    return TTX_OK;
}
// bytes of the state store of a gradient call, from the environment (read on every call) or the default
static size_t env_grad_store()
{
    if (const char *e = getenv("TTX_BASIS_GRAD_STORE")) { const long long v = atoll(e); if (v >= 1) return (size_t)v; }
    return TTX_BG_STORE_DEFAULT;
}
enum { BGM_TABLE, BGM_BACK, BGM_FWD };      // OpMarks phases of a call, BgLast::ms takes the sums
// in: the coordinates, or the caller's phi with din its dphi; val may be null
static int bg_run(ttx_engine *h, const char *who, BsSrc src, int64_t npts, const double *in, const double *din, const ttx_basis *basis, double *val, double *grad, int32_t mode)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (npts < 0 || (npts > 0 && (!in || !grad || (tab ? !din : !basis)))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    const int d = h->d;
    if (!tab && basis) for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    const BgPlan pl = bg_plan(d, h->n1.data() + 1, h->rfinal.data(), dev_ncu(h), src, npts, mode, env_chunk("TTX_BASIS_CHUNK", op_chunk_default(h->RM)), env_grad_store());
    if (pl.refusal == BS_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.rmax);
    if (pl.refusal == BS_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    h->bg = BgLast();
    h->bg.flops = pl.flops; h->bg.mode = pl.eff; h->bg.chunk = (int64_t)pl.chunk;
    if (npts == 0) return TTX_OK;
    EvTrain T;
    if ((rc = ev_train(h, &T))) return rc;
    // the nodes of the LINEAR modes, one device block
    std::vector<BsMode> M(d);
    if (!tab) {
        OpMeta meta(h->meta_host);
        std::vector<size_t> o_nodes(d, 0);
        for (int k = 0; k < d; k++)
            if (basis[k].kind == TTX_BASIS_LINEAR) o_nodes[k] = meta.put(std::vector<double>(basis[k].nodes, basis[k].nodes + h->n1[k + 1]));
        char *dm = nullptr;
        if (!meta.host.empty() && (rc = meta.upload(h, SC_META, &dm))) return rc;
        for (int k = 0; k < d; k++) {
            const ttx_basis &b = basis[k];
            const bool cosk = b.kind == TTX_BASIS_COS;
            M[k] = BsMode{b.kind, b.flags, h->n1[k + 1], cosk ? b.a : 0.0, cosk ? ttx_basis_cos_w(b.a, b.b) : 0.0, cosk ? nullptr : (const double *)(dm + o_nodes[k])};
        }
    }
    if ((rc = buf_reserve(h, {{SC_XA, pl.b_xa}, {SC_XB, pl.b_xb}, {SC_BTAB, pl.b_btab}, {SC_X, pl.b_x}, {SC_OUT, pl.b_out}, {SC_GST, pl.b_gst}}))) return rc;
    double *btab = buf<double>(h, SC_BTAB), *dtab = btab + pl.chunk * pl.nmax, *sin_ = buf<double>(h, SC_X), *sout = buf<double>(h, SC_OUT);
    double *gst = buf<double>(h, SC_GST), *XA = buf<double>(h, SC_XA), *XB = buf<double>(h, SC_XB);
    OpMarks marks(h->op_ev);
    for (int64_t o = 0; o < npts; o += (int64_t)pl.chunk) {
        const int c = (int)std::min<int64_t>((int64_t)pl.chunk, npts - o);
        const double *cin = in + (size_t)o * pl.row, *cdin = tab ? din + (size_t)o * pl.row : nullptr;
        double *cval = val ? val + o : nullptr, *cgrad = grad + (size_t)o * d;
        if (!dev) {
            HIPCHECK(hipMemcpyAsync(sin_, cin, sizeof(double) * (size_t)c * pl.row, hipMemcpyHostToDevice, h->stream));
            cin = sin_;
            if (tab) {
                HIPCHECK(hipMemcpyAsync(sin_ + pl.chunk * pl.row, cdin, sizeof(double) * (size_t)c * pl.row, hipMemcpyHostToDevice, h->stream));
                cdin = sin_ + pl.chunk * pl.row;
            }
            cval = val ? sout : nullptr; cgrad = sout + pl.chunk;
        }
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        // the table of mode i where the call forms it (dphi only on the way back), else the caller's rows
        const double *ph = nullptr, *dh = nullptr;
        size_t ld = 0;
        auto tables = [&](int i, bool both) {
            ph = cin + pl.off[i]; dh = tab ? cdin + pl.off[i] : nullptr; ld = pl.sumn;
            if (tab) return TTX_OK;
            hipLaunchKernelGGL(k_bg_table, g1((size_t)c * M[i].n), dim3(256), 0, h->stream, M[i], (long long)c, cin + i, d, btab, both ? dtab : (double *)nullptr);
            ph = btab; dh = dtab; ld = (size_t)M[i].n;
            return marks.mark(h->stream, BGM_TABLE);
        };
        double *X = XA, *Z = XB;
        for (int i = d - 1; i >= 0; i--) {                                      // backward: z and e of every mode, D_i into the store
            if ((rc = tables(i, true))) return rc;
            const double *Xin = i == d - 1 ? nullptr : X;
            double *Di = gst + pl.soff[i] * pl.chunk;
            const int last = i == 0;
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bg_exact_back, dim3(pl.g_exact(c)), dim3(256), pl.lds_back, h->stream, T, i, (long long)c, ph, dh, ld, Xin, Z, Di, cval, last);
            else
                with_tier<true>(pl.step[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL((k_bg_gemm<decltype(mr)::value, false>), dim3(pl.g_back(i, c)), dim3(256), pl.step[i].lds_back, h->stream,
                                       T, i, c, ph, dh, ld, Xin, Z, Di, cval, (double *)nullptr, d, last);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, BGM_BACK))) return rc;
            std::swap(X, Z);
        }
        X = XA; Z = XB;
        for (int i = 0; i < d; i++) {                                           // forward: grad_i = l . D_i, then l through mode i
            const int last = i == d - 1;
            if (!last) { if ((rc = tables(i, false))) return rc; } else { ph = cin; ld = 0; }     // mode d forms no new state: no table is read
            const double *Lin = i == 0 ? nullptr : X;
            double *Di = gst + pl.soff[i] * pl.chunk;
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bg_exact_fwd, dim3(pl.g_exact(c)), dim3(256), pl.lds_fwd, h->stream, T, i, (long long)c, ph, ld, Lin, Z, Di, cgrad, d, last);
            else
                with_tier<true>(pl.step[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL((k_bg_gemm<decltype(mr)::value, true>), dim3(pl.g_fwd(i, c)), dim3(256), pl.step[i].lds_fwd, h->stream,
                                       T, i, c, ph, (const double *)nullptr, ld, Lin, Z, Di, (double *)nullptr, cgrad, d, last);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, BGM_FWD))) return rc;
            std::swap(X, Z);
        }
        if (!dev) {
            if (val) HIPCHECK(hipMemcpyAsync(val + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
            HIPCHECK(hipMemcpyAsync(grad + (size_t)o * d, sout + pl.chunk, sizeof(double) * (size_t)c * d, hipMemcpyDeviceToHost, h->stream));
        }
        if (!dev || marks.phase.size() > 4096) {                                // the staging blocks are reused by the next chunk; the event chain stays short
            HIPCHECK(hipStreamSynchronize(h->stream));
            if ((rc = marks.sum(h->bg.ms))) return rc;
        }
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = marks.sum(h->bg.ms))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_basis_grad_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, double *val, double *grad, int32_t mode)
{
    return bg_run(h, "ttx_basis_grad_batch", BS_X_HOST, npts, x, nullptr, basis, val, grad, mode);
}
extern "C" int ttx_basis_grad_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, double *val_dev, double *grad_dev, int32_t mode)
{
    return bg_run(h, "ttx_basis_grad_batch_dev", BS_X_DEV, npts, x_dev, nullptr, basis, val_dev, grad_dev, mode);
}
extern "C" int ttx_basis_grad_tab(ttx_engine *h, int64_t npts, const double *phi, const double *dphi, double *val, double *grad, int32_t mode)
{
    return bg_run(h, "ttx_basis_grad_tab", BS_TAB_HOST, npts, phi, dphi, nullptr, val, grad, mode);
}
extern "C" int ttx_basis_grad_tab_dev(ttx_engine *h, int64_t npts, const double *phi_dev, const double *dphi_dev, double *val_dev, double *grad_dev, int32_t mode)
{
    return bg_run(h, "ttx_basis_grad_tab_dev", BS_TAB_DEV, npts, phi_dev, dphi_dev, nullptr, val_dev, grad_dev, mode);
}
extern "C" int ttx_basis_grad_last(const ttx_engine *h, double *ms_table, double *ms_back, double *ms_fwd, double *flops, int32_t *mode_ran, int64_t *chunk_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_basis_grad_last: null engine");
    if (ms_table) *ms_table = h->bg.ms[BGM_TABLE];
    if (ms_back) *ms_back = h->bg.ms[BGM_BACK];
    if (ms_fwd) *ms_fwd = h->bg.ms[BGM_FWD];
    if (flops) *flops = h->bg.flops;
    if (mode_ran) *mode_ran = h->bg.mode;
    if (chunk_ran) *chunk_ran = h->bg.chunk;
    return TTX_OK;
}

// ---- gradient with respect to the cores of the train in a function basis (ttx_basis_core_grad.h) ---------------------------------
enum { CGM_TABLE, CGM_BACK, CGM_FWD, CGM_ACC };     // OpMarks phases of a call, CgLast::ms takes the sums
// what ttx_basis_batch refuses of the train itself, asked before anything is touched
static int cg_check_train(ttx_engine *h, const char *who)
{
    const int rmax = *std::max_element(h->rfinal.begin(), h->rfinal.begin() + h->d + 1);
    if (rmax > 128) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, rmax);
    if (h->rfinal[0] != 1 || h->rfinal[h->d] != 1) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    return TTX_OK;
}
// in: the coordinates or the caller's phi; cw: the weights c; val may be null; g: the packed gradient, on the host unless dev
static int cg_run(ttx_engine *h, const char *who, BsSrc src, int64_t npts, const double *in, const ttx_basis *basis, const double *cw, double *val, double *g,
                  int32_t accumulate, int32_t mode)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (npts < 0 || (npts > 0 && (!in || !cw || !g || (!tab && !basis)))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    if (accumulate != 0 && accumulate != 1) return fail(TTX_EINVAL, "%s: accumulate is 0 or 1 (got %d)", who, accumulate);
    const int d = h->d;
    if (!tab && basis) for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    const CgPlan pl = cg_plan(d, h->n1.data() + 1, h->rfinal.data(), dev_ncu(h), src, !dev, npts, mode, env_chunk("TTX_BASIS_CHUNK", op_chunk_default(h->RM)), env_grad_store());
    if (pl.refusal == BS_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.rmax);
    if (pl.refusal == BS_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    h->cg = CgLast();
    h->cg.flops = pl.flops; h->cg.mode = pl.eff; h->cg.chunk = (int64_t)pl.chunk;
    if (npts == 0) {                                                            // no chain: accumulate == 0 writes 0.0 to all of g, accumulate == 1 touches nothing
        if (accumulate || !g) return TTX_OK;
        if (!dev) { std::fill(g, g + pl.gsize, 0.0); return TTX_OK; }
        HIPCHECK(hipMemsetAsync(g, 0, sizeof(double) * pl.gsize, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        return TTX_OK;
    }
    EvTrain T;
    if ((rc = ev_train(h, &T))) return rc;
    // the nodes of the LINEAR modes, one device block
    std::vector<BsMode> M(d);
    if (!tab) {
        OpMeta meta(h->meta_host);
        std::vector<size_t> o_nodes(d, 0);
        for (int k = 0; k < d; k++)
            if (basis[k].kind == TTX_BASIS_LINEAR) o_nodes[k] = meta.put(std::vector<double>(basis[k].nodes, basis[k].nodes + h->n1[k + 1]));
        char *dm = nullptr;
        if (!meta.host.empty() && (rc = meta.upload(h, SC_META, &dm))) return rc;
        for (int k = 0; k < d; k++) {
            const ttx_basis &b = basis[k];
            const bool cosk = b.kind == TTX_BASIS_COS;
            M[k] = BsMode{b.kind, b.flags, h->n1[k + 1], cosk ? b.a : 0.0, cosk ? ttx_basis_cos_w(b.a, b.b) : 0.0, cosk ? nullptr : (const double *)(dm + o_nodes[k])};
        }
    }
    if ((rc = buf_reserve(h, {{SC_XA, pl.b_xa}, {SC_XB, pl.b_xb}, {SC_BTAB, pl.b_btab}, {SC_X, pl.b_x}, {SC_OUT, pl.b_out}, {SC_GST, pl.b_gst}, {SC_CGG, pl.b_cgg}, {SC_CGP, pl.b_part}}))) return rc;
    double *btab = buf<double>(h, SC_BTAB), *sin_ = buf<double>(h, SC_X), *sout = buf<double>(h, SC_OUT);
    double *gst = buf<double>(h, SC_GST), *XA = buf<double>(h, SC_XA), *XB = buf<double>(h, SC_XB), *part = buf<double>(h, SC_CGP);
    double *G = dev ? g : buf<double>(h, SC_CGG);
    // G0: the caller's block, or 0.0; every chunk then continues from the buffer
    if (!accumulate) HIPCHECK(hipMemsetAsync(G, 0, sizeof(double) * pl.gsize, h->stream));
    else if (!dev) HIPCHECK(hipMemcpyAsync(G, g, sizeof(double) * pl.gsize, hipMemcpyHostToDevice, h->stream));
    OpMarks marks(h->op_ev);
    for (int64_t o = 0; o < npts; o += (int64_t)pl.chunk) {
        const int c = (int)std::min<int64_t>((int64_t)pl.chunk, npts - o);
        const double *cin = in + (size_t)o * pl.row, *cc = cw + o;
        double *cval = val ? val + o : XA;                                      // nobody's val: mode 1's launch still writes one number per point, into a state buffer the forward pass overwrites
        if (!dev) {
            HIPCHECK(hipMemcpyAsync(sin_, cin, sizeof(double) * (size_t)c * pl.row, hipMemcpyHostToDevice, h->stream));
            HIPCHECK(hipMemcpyAsync(sin_ + pl.chunk * pl.row, cc, sizeof(double) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            cin = sin_; cc = sin_ + pl.chunk * pl.row;
            if (val) cval = sout;
        }
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        const double *ph = nullptr;
        size_t ld = 0;
        auto tables = [&](int i) {
            ph = cin + pl.off[i]; ld = pl.sumn;
            if (tab) return TTX_OK;
            hipLaunchKernelGGL(k_bg_table, g1((size_t)c * M[i].n), dim3(256), 0, h->stream, M[i], (long long)c, cin + i, d, btab, (double *)nullptr);
            ph = btab; ld = (size_t)M[i].n;
            return marks.mark(h->stream, CGM_TABLE);
        };
        auto Xof = [&](int bond) { return gst + pl.soff(bond) * pl.chunk; };     // X_bond, bond = 1 .. d-1
        for (int i = d - 1; i >= 0; i--) {                                      // backward: the value chain, every state into the store
            if ((rc = tables(i))) return rc;
            const double *Xin = i == d - 1 ? nullptr : Xof(i + 1);
            double *Z = i == 0 ? XB : Xof(i), *o1 = i == 0 ? cval : nullptr;    // mode 1 writes no state
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bs_exact, dim3(pl.g_exact(c)), dim3(256), pl.lds_back, h->stream, T, i, (long long)c, ph, ld, Xin, Z, o1);
            else
                with_tier<true>(pl.back[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL(k_bs_gemm<decltype(mr)::value>, dim3(pl.g_back(i, c)), dim3(256), pl.back[i].lds, h->stream, T, i, c, ph, ld, Xin, Z, o1);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, CGM_BACK))) return rc;
        }
        double *X = XA, *Z = XB;
        for (int i = 0; i < d; i++) {                                           // forward: G_i from L_i and X_i, then L through mode i
            if ((rc = tables(i))) return rc;
            const double *Lin = i == 0 ? nullptr : X, *Xi = i == d - 1 ? nullptr : Xof(i + 1);
            const int r0 = h->rfinal[i], n = h->n1[i + 1], r1 = h->rfinal[i + 1];
            const CgStep &st = pl.step[i];
            double *Gi = G + st.goff;
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_cg_exact, dim3((unsigned)((st.size + 255) / 256)), dim3(256), 0, h->stream, r0, n, r1, (long long)c, cc, ph, ld, Lin, Xi, pl.ldx, Gi);
            else {
                const int ns = pl.nsplit(i, c);
                with_tier<true>(st.tier, [&](auto mr) {
                    hipLaunchKernelGGL(k_cg_gemm<decltype(mr)::value>, dim3(st.ngrp, ns), dim3(256), st.lds, h->stream, r0, n, r1, c, st.seg, cc, ph, ld, Lin, Xi, pl.ldx, part);
                    return 0;
                });
                hipLaunchKernelGGL(k_cg_reduce, g1(st.size), dim3(256), 0, h->stream, (long long)st.size, ns, part, Gi);
            }
            if ((rc = marks.mark(h->stream, CGM_ACC))) return rc;
            if (i == d - 1) break;                                              // L_(d+1) is not formed
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bg_exact_fwd, dim3(pl.g_exact(c)), dim3(256), pl.lds_fwd, h->stream, T, i, (long long)c, ph, ld, Lin, Z, (const double *)nullptr, (double *)nullptr, d, 0);
            else
                with_tier<true>(pl.fwd[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL((k_bg_gemm<decltype(mr)::value, true>), dim3(pl.g_fwd(i, c)), dim3(256), pl.fwd[i].lds_fwd, h->stream,
                                       T, i, c, ph, (const double *)nullptr, ld, Lin, Z, (double *)nullptr, (double *)nullptr, (double *)nullptr, d, 0);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, CGM_FWD))) return rc;
            std::swap(X, Z);
        }
        if (!dev && val) HIPCHECK(hipMemcpyAsync(val + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
        if (!dev || marks.phase.size() > 4096) {                                // the staging blocks are reused by the next chunk; the event chain stays short
            HIPCHECK(hipStreamSynchronize(h->stream));
            if ((rc = marks.sum(h->cg.ms))) return rc;
        }
    }
    if (!dev) HIPCHECK(hipMemcpyAsync(g, G, sizeof(double) * pl.gsize, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = marks.sum(h->cg.ms))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_basis_core_grad_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, const double *c, double *val, double *g, int32_t accumulate, int32_t mode)
{
    return cg_run(h, "ttx_basis_core_grad_batch", BS_X_HOST, npts, x, basis, c, val, g, accumulate, mode);
}
extern "C" int ttx_basis_core_grad_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *c_dev, double *val_dev, double *g_dev, int32_t accumulate, int32_t mode)
{
    return cg_run(h, "ttx_basis_core_grad_batch_dev", BS_X_DEV, npts, x_dev, basis, c_dev, val_dev, g_dev, accumulate, mode);
}
extern "C" int ttx_basis_core_grad_tab(ttx_engine *h, int64_t npts, const double *phi, const double *c, double *val, double *g, int32_t accumulate, int32_t mode)
{
    return cg_run(h, "ttx_basis_core_grad_tab", BS_TAB_HOST, npts, phi, nullptr, c, val, g, accumulate, mode);
}
extern "C" int ttx_basis_core_grad_tab_dev(ttx_engine *h, int64_t npts, const double *phi_dev, const double *c_dev, double *val_dev, double *g_dev, int32_t accumulate, int32_t mode)
{
    return cg_run(h, "ttx_basis_core_grad_tab_dev", BS_TAB_DEV, npts, phi_dev, nullptr, c_dev, val_dev, g_dev, accumulate, mode);
}
extern "C" int ttx_basis_core_grad_last(const ttx_engine *h, double *ms_table, double *ms_back, double *ms_fwd, double *ms_acc, double *flops, int32_t *mode_ran, int64_t *chunk_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_basis_core_grad_last: null engine");
    if (ms_table) *ms_table = h->cg.ms[CGM_TABLE];
    if (ms_back) *ms_back = h->cg.ms[CGM_BACK];
    if (ms_fwd) *ms_fwd = h->cg.ms[CGM_FWD];
    if (ms_acc) *ms_acc = h->cg.ms[CGM_ACC];
    if (flops) *flops = h->cg.flops;
    if (mode_ran) *mode_ran = h->cg.mode;
    if (chunk_ran) *chunk_ran = h->cg.chunk;
    return TTX_OK;
}

// ---- ranks grown from data: gradient enrichment (ttx_basis_enrich.h) --------------------------------------------------------------
enum { ENM_TABLE, ENM_BACK, ENM_SKETCH, ENM_QR, ENM_ASM };      // OpMarks phases of a call, EnLast::ms takes the sums
// the passes of a call: Y (the packed sketches, zeroed by the caller) takes every bond's sum over all points
static int en_sketch(ttx_engine *h, const EnPlan &pl, BsSrc src, int64_t npts, const double *in, const ttx_basis *basis, const double *cw, unsigned long long seed, double *Y)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    const CgPlan &g = pl.cg;
    const int d = h->d;
    int rc;
    EvTrain T;
    if ((rc = ev_train(h, &T))) return rc;
    T.ldx = g.ldx;                                                              // every state row of this call at the plan's stride
    std::vector<BsMode> M(d);
    if (!tab) {
        OpMeta meta(h->meta_host);
        std::vector<size_t> o_nodes(d, 0);
        for (int k = 0; k < d; k++)
            if (basis[k].kind == TTX_BASIS_LINEAR) o_nodes[k] = meta.put(std::vector<double>(basis[k].nodes, basis[k].nodes + h->n1[k + 1]));
        char *dm = nullptr;
        if (!meta.host.empty() && (rc = meta.upload(h, SC_META, &dm))) return rc;
        for (int k = 0; k < d; k++) {
            const ttx_basis &b = basis[k];
            const bool cosk = b.kind == TTX_BASIS_COS;
            M[k] = BsMode{b.kind, b.flags, h->n1[k + 1], cosk ? b.a : 0.0, cosk ? ttx_basis_cos_w(b.a, b.b) : 0.0, cosk ? nullptr : (const double *)(dm + o_nodes[k])};
        }
    }
    if ((rc = buf_reserve(h, {{SC_XA, g.b_xa}, {SC_XB, g.b_xb}, {SC_BTAB, g.b_btab}, {SC_X, g.b_x}, {SC_GST, g.b_gst}, {SC_CGP, pl.b_part}}))) return rc;
    double *btab = buf<double>(h, SC_BTAB), *sin_ = buf<double>(h, SC_X);
    double *gst = buf<double>(h, SC_GST), *XA = buf<double>(h, SC_XA), *XB = buf<double>(h, SC_XB), *part = buf<double>(h, SC_CGP);
    double *zb = gst + pl.zoff() * g.chunk;
    OpMarks marks(h->op_ev);
    for (int64_t o = 0; o < npts; o += (int64_t)g.chunk) {
        const int c = (int)std::min<int64_t>((int64_t)g.chunk, npts - o);
        const double *cin = in + (size_t)o * g.row, *cc = cw + o;
        if (!dev) {
            HIPCHECK(hipMemcpyAsync(sin_, cin, sizeof(double) * (size_t)c * g.row, hipMemcpyHostToDevice, h->stream));
            HIPCHECK(hipMemcpyAsync(sin_ + g.chunk * g.row, cc, sizeof(double) * (size_t)c, hipMemcpyHostToDevice, h->stream));
            cin = sin_; cc = sin_ + g.chunk * g.row;
        }
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        const double *ph = nullptr;
        size_t ld = 0;
        auto tables = [&](int i) {
            ph = cin + g.off[i]; ld = g.sumn;
            if (tab) return TTX_OK;
            hipLaunchKernelGGL(k_bg_table, g1((size_t)c * M[i].n), dim3(256), 0, h->stream, M[i], (long long)c, cin + i, d, btab, (double *)nullptr);
            ph = btab; ld = (size_t)M[i].n;
            return marks.mark(h->stream, ENM_TABLE);
        };
        auto Xof = [&](int bond) { return gst + g.soff(bond) * g.chunk; };      // X_bond, bond = 1 .. d-1
        for (int i = d - 1; i >= 1; i--) {                                      // backward: the value chain down to X_1, every state into the store
            if ((rc = tables(i))) return rc;
            const double *Xin = i == d - 1 ? nullptr : Xof(i + 1);
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bs_exact, dim3(g.g_exact(c)), dim3(256), g.lds_back, h->stream, T, i, (long long)c, ph, ld, Xin, Xof(i), (double *)nullptr);
            else
                with_tier<true>(g.back[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL(k_bs_gemm<decltype(mr)::value>, dim3(g.g_back(i, c)), dim3(256), g.back[i].lds, h->stream, T, i, c, ph, ld, Xin, Xof(i), (double *)nullptr);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, ENM_BACK))) return rc;
        }
        int last = 0;                                                           // the last bond that takes a direction: L is advanced no further
        for (int b = 1; b < d; b++) if (pl.step[b].k) last = b;
        double *X = XA, *Z = XB;
        for (int i = 0; i < last; i++) {                                        // forward, bond b = i + 1: z, then Y_b from L_b and z, then L through mode i
            const int b = i + 1;
            const EnStep &st = pl.step[b];
            const double *Lin = i == 0 ? nullptr : X;
            if (st.k) {
                const int n2 = h->n1[b + 1], r2 = h->rfinal[b + 1];
                const double *X2 = b == d - 1 ? nullptr : Xof(b + 1);
                if ((rc = tables(b))) return rc;
                if (pl.eff == TTX_EVAL_EXACT)
                    hipLaunchKernelGGL(k_en_z_exact, dim3(g.g_exact(c)), dim3(256), 0, h->stream, seed, b, st.k, n2, r2, (long long)c, ph, ld, X2, g.ldx, zb);
                else
                    with_tier(st.qt, [&](auto qt) {
                        hipLaunchKernelGGL(k_en_z_gemm<decltype(qt)::value>, dim3(pl.g_z(b, c)), dim3(256), 0, h->stream, seed, b, st.k, n2, r2, c, ph, ld, X2, g.ldx, zb);
                        return 0;
                    });
                if ((rc = marks.mark(h->stream, ENM_SKETCH)) || (rc = tables(i))) return rc;
                const int r0 = h->rfinal[i], n = h->n1[i + 1];
                double *Yb = Y + st.acc.goff;
                if (pl.eff == TTX_EVAL_EXACT)
                    hipLaunchKernelGGL(k_cg_exact, dim3((unsigned)((st.acc.size + 255) / 256)), dim3(256), 0, h->stream, r0, n, st.k, (long long)c, cc, ph, ld, Lin, (const double *)zb, g.ldx, Yb);
                else {
                    const int ns = pl.nsplit(b, c);
                    with_tier<true>(st.acc.tier, [&](auto mr) {
                        hipLaunchKernelGGL(k_cg_gemm<decltype(mr)::value>, dim3(st.acc.ngrp, ns), dim3(256), st.acc.lds, h->stream, r0, n, st.k, c, st.acc.seg, cc, ph, ld, Lin, (const double *)zb, g.ldx, part);
                        return 0;
                    });
                    hipLaunchKernelGGL(k_cg_reduce, g1(st.acc.size), dim3(256), 0, h->stream, (long long)st.acc.size, ns, part, Yb);
                }
                if ((rc = marks.mark(h->stream, ENM_SKETCH))) return rc;
            }
            if (b == last) break;
            if (!st.k && (rc = tables(i))) return rc;
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_bg_exact_fwd, dim3(g.g_exact(c)), dim3(256), g.lds_fwd, h->stream, T, i, (long long)c, ph, ld, Lin, Z, (const double *)nullptr, (double *)nullptr, d, 0);
            else
                with_tier<true>(g.fwd[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL((k_bg_gemm<decltype(mr)::value, true>), dim3(g.g_fwd(i, c)), dim3(256), g.fwd[i].lds_fwd, h->stream,
                                       T, i, c, ph, (const double *)nullptr, ld, Lin, Z, (double *)nullptr, (double *)nullptr, (double *)nullptr, d, 0);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, ENM_SKETCH))) return rc;
            std::swap(X, Z);
        }
        if (!dev || marks.phase.size() > 4096) {                                // the staging blocks are reused by the next chunk; the event chain stays short
            HIPCHECK(hipStreamSynchronize(h->stream));
            if ((rc = marks.sum(h->en.ms))) return rc;
        }
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    return marks.sum(h->en.ms);
}
// everything of the call that works on the new engine e: the QR of every bond that takes directions, then all cores in one launch.  The
// launches go to h's stream (e runs on it for the length of the call); Y gives way to the new directions bond by bond
static int en_fill(ttx_engine *h, ttx_engine *e, const EnPlan &pl, const std::vector<int> &added, const std::vector<int> &ex, double *Y, double *gain)
{
    const int d = h->d;
    int rc;
    if ((rc = tt_prepare(e, "ttx_basis_enrich"))) return rc;
    struct OnStream { ttx_engine *e; hipStream_t own; ~OnStream() { e->stream = own; } } on{e, e->stream};
    e->stream = h->stream;
    hipStream_t st = h->stream;
    const TtScratch s(e);
    OpMarks marks(h->op_ev);
    if ((rc = marks.mark(st, OpMarks::DISCARD))) return rc;
    std::vector<double> rdiag((size_t)(d - 1) * 128, 0.0);
    for (int b = 1; b < d; b++) {
        if (!added[b]) continue;
        const EnStep &sp = pl.step[b];
        double *Yb = Y + sp.acc.goff;
        hipLaunchKernelGGL(k_en_pack, g1((size_t)sp.rows * sp.cols), dim3(256), 0, st, (const double *)core_dev(h, b), h->RM, h->P.SS, h->rfinal[b - 1], h->n1[b], h->rfinal[b], sp.k,
                           (const double *)Yb, ex[b], e->Wa);
        if ((rc = qr(e, sp.rows, sp.cols, e->Wa, s.Rm, s.tau))) return rc;
        const int r1 = h->rfinal[b];
        HIPCHECK(hipMemcpyAsync(Yb, e->Wa + (size_t)sp.rows * r1, sizeof(double) * sp.acc.size, hipMemcpyDeviceToDevice, st));       // Q_b = the columns r1 .. r1 + k - 1
        HIPCHECK(hipMemcpy2DAsync(rdiag.data() + (size_t)(b - 1) * 128, sizeof(double), s.Rm + (size_t)r1 * (sp.cols + 1), sizeof(double) * (sp.cols + 1), sizeof(double), sp.k,
                                  hipMemcpyDeviceToHost, st));                  // R(r1 + q, r1 + q), R with the leading dimension cols
        HIPCHECK(hipStreamSynchronize(st));                                     // the pageable rows have landed before Rm is written again
    }
    if ((rc = marks.mark(st, ENM_QR))) return rc;
    std::vector<EnCore> cs(d);
    long long tot = 0;
    for (int k = 1; k <= d; k++) {
        EnCore &C = cs[k - 1];
        C.U = core_dev(h, k); C.dst = core_dev(e, k); C.Q = k < d ? Y + pl.step[k].acc.goff : nullptr;
        C.first = tot; C.r0 = h->rfinal[k - 1]; C.n = h->n1[k]; C.r1 = h->rfinal[k]; C.R0 = e->rfinal[k - 1]; C.R1 = e->rfinal[k];
        tot += (long long)C.R0 * C.n * C.R1;
    }
    OpMeta meta(h->meta_host);
    meta.put(cs);
    char *dm;
    if ((rc = meta.upload(h, SC_META, &dm))) return rc;
    hipLaunchKernelGGL(k_en_assemble, g1((size_t)tot), dim3(256), 0, st, (const EnCore *)dm, d, tot, h->RM, h->P.SS, e->RM, e->P.SS);
    if ((rc = marks.mark(st, ENM_ASM))) return rc;
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipGetLastError());
    if ((rc = marks.sum(h->en.ms))) return rc;
    if (gain) for (int b = 1; b < d; b++) for (int q = 0; q < added[b]; q++) gain[(size_t)(b - 1) * 128 + q] = ldexp(fabs(rdiag[(size_t)(b - 1) * 128 + q]), ex[b]);
    return TTX_OK;
}
// in: the coordinates or the caller's phi; cw: the weights c; y (optional): on the device where dev, the other outputs on the host
static int en_run(ttx_engine *h, const char *who, BsSrc src, int64_t npts, const double *in, const ttx_basis *basis, const double *cw, const int32_t *add, uint64_t seed,
                  int32_t mode, ttx_engine **out, int32_t *added_out, double *gain, double *ynorm2, double *y)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    if (out) *out = nullptr;
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!out || !add) return fail(TTX_EINVAL, "%s: null add or out", who);
    if (npts < 0 || (npts > 0 && (!in || !cw || (!tab && !basis)))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    const int d = h->d;
    if (d < 2) return fail(TTX_EINVAL, "%s: at least two cores are needed (got %d)", who, d);
    for (int b = 1; b < d; b++) if (add[b - 1] < 0) return fail(TTX_EINVAL, "%s: add(%d)=%d is negative", who, b, (int)add[b - 1]);
    if (!tab && basis) for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    double auto_flops = TTX_EN_AUTO_FLOPS;
    if (const char *e = getenv("TTX_ENRICH_AUTO_FLOPS")) { const double v = atof(e); if (v > 0.0) auto_flops = v; }
    const EnPlan pl = en_plan(d, h->n1.data() + 1, h->rfinal.data(), add, dev_ncu(h), src, npts, mode, env_chunk("TTX_BASIS_CHUNK", op_chunk_default(h->RM)), env_grad_store(), auto_flops);
    if (pl.refusal == BS_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.cg.rmax);
    if (pl.refusal == BS_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    if (pl.storage_bond)
        return fail(TTX_EINVAL, "%s: the rank at bond %d grows to %d, and %d times the largest mode is more than a new engine stores (maxrank*n too large: lower add)", who,
                    pl.storage_bond, pl.storage_rank, pl.storage_rank);
    h->en = EnLast();
    h->en.flops = pl.flops; h->en.mode = pl.eff; h->en.chunk = (int64_t)pl.cg.chunk;
    const int nb = d - 1;
    if ((rc = buf_reserve(h, {{SC_ENY, pl.b_y}, {SC_ENS, pl.b_stat}}))) return rc;
    double *Y = buf<double>(h, SC_ENY), *stat = buf<double>(h, SC_ENS);
    HIPCHECK(hipMemsetAsync(Y, 0, pl.b_y, h->stream));
    std::vector<int> added(d + 1, 0), ex(d + 1, 0);
    std::vector<double> norm2(nb, 0.0), mx(nb, 0.0);
    if (pl.sketch) {
        if ((rc = en_sketch(h, pl, src, npts, in, basis, cw, (unsigned long long)seed, Y))) return rc;
        // step 5: per bond the sum of squares by ttx_cores_dot's rule and the largest |Y|, the 256 segment results folded here
        std::vector<size_t> off(d, 0);
        for (int b = 1; b < d; b++) off[b] = off[b - 1] + pl.step[b].acc.size;
        OpMeta meta(h->meta_host);
        meta.put(off);
        char *dm;
        if ((rc = meta.upload(h, SC_META, &dm))) return rc;
        OpMarks marks(h->op_ev);
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        hipLaunchKernelGGL(k_en_stat, dim3(256, nb), dim3(256), 0, h->stream, (const size_t *)dm, (const double *)Y, stat, stat + (size_t)256 * nb);
        if ((rc = marks.mark(h->stream, ENM_SKETCH))) return rc;
        std::vector<double> hs((size_t)2 * 256 * nb);
        HIPCHECK(hipMemcpyAsync(hs.data(), stat, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        HIPCHECK(hipGetLastError());
        if ((rc = marks.sum(h->en.ms))) return rc;
        for (int b = 1; b < d; b++) {
            double s = 0.0, m = 0.0;
            for (int k = 0; k < 256; k++) { s = s + hs[(size_t)256 * (b - 1) + k]; m = std::max(m, hs[(size_t)256 * (nb + b - 1) + k]); }
            norm2[b - 1] = s; mx[b - 1] = m;
            if (m > 0.0 && std::isfinite(m)) { added[b] = pl.step[b].k; (void)frexp(m, &ex[b]); }
        }
    }
    if (y && pl.ysize) HIPCHECK(hipMemcpyAsync(y, Y, sizeof(double) * pl.ysize, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    std::vector<double> hgain((size_t)nb * 128, 0.0);
    for (int b = 1; b < d; b++) if (pl.step[b].k && !std::isfinite(mx[b - 1])) std::fill(hgain.begin() + (size_t)(b - 1) * 128, hgain.begin() + (size_t)b * 128, NAN);
    std::vector<int32_t> nn = modes_of(h), rr(d + 1, 1);
    for (int b = 1; b < d; b++) rr[b] = h->rfinal[b] + added[b];
    rc = new_train(out, who, d, nn.data(), rr.data(), h->cfg.device, [&](ttx_engine *e) { return en_fill(h, e, pl, added, ex, Y, hgain.data()); });
    if (rc) return rc;
    if (added_out) for (int b = 1; b < d; b++) added_out[b - 1] = added[b];
    if (gain) std::copy(hgain.begin(), hgain.end(), gain);
    if (ynorm2) std::copy(norm2.begin(), norm2.end(), ynorm2);
    return TTX_OK;
}
extern "C" int ttx_basis_enrich_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, const double *c, const int32_t *add, uint64_t seed, int32_t mode,
                                      ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y)
{
    return en_run(h, "ttx_basis_enrich_batch", BS_X_HOST, npts, x, basis, c, add, seed, mode, out, added, gain, ynorm2, y);
}
extern "C" int ttx_basis_enrich_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *c_dev, const int32_t *add, uint64_t seed, int32_t mode,
                                          ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y_dev)
{
    return en_run(h, "ttx_basis_enrich_batch_dev", BS_X_DEV, npts, x_dev, basis, c_dev, add, seed, mode, out, added, gain, ynorm2, y_dev);
}
extern "C" int ttx_basis_enrich_tab(ttx_engine *h, int64_t npts, const double *phi, const double *c, const int32_t *add, uint64_t seed, int32_t mode,
                                    ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y)
{
    return en_run(h, "ttx_basis_enrich_tab", BS_TAB_HOST, npts, phi, nullptr, c, add, seed, mode, out, added, gain, ynorm2, y);
}
extern "C" int ttx_basis_enrich_tab_dev(ttx_engine *h, int64_t npts, const double *phi_dev, const double *c_dev, const int32_t *add, uint64_t seed, int32_t mode,
                                        ttx_engine **out, int32_t *added, double *gain, double *ynorm2, double *y_dev)
{
    return en_run(h, "ttx_basis_enrich_tab_dev", BS_TAB_DEV, npts, phi_dev, nullptr, c_dev, add, seed, mode, out, added, gain, ynorm2, y_dev);
}
extern "C" int ttx_basis_enrich_last(const ttx_engine *h, double *ms_table, double *ms_back, double *ms_sketch, double *ms_qr, double *ms_asm, double *flops, int32_t *mode_ran,
                                     int64_t *chunk_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_basis_enrich_last: null engine");
    if (ms_table) *ms_table = h->en.ms[ENM_TABLE];
    if (ms_back) *ms_back = h->en.ms[ENM_BACK];
    if (ms_sketch) *ms_sketch = h->en.ms[ENM_SKETCH];
    if (ms_qr) *ms_qr = h->en.ms[ENM_QR];
    if (ms_asm) *ms_asm = h->en.ms[ENM_ASM];
    if (flops) *flops = h->en.flops;
    if (mode_ran) *mode_ran = h->en.mode;
    if (chunk_ran) *chunk_ran = h->en.chunk;
    return TTX_OK;
}
// U_i <- U_i + alpha[i - 1] G_i for every core in one launch; g: the packed blocks, on the host unless dev.  The engine keeps nothing
// that is derived from the cores between two calls (every operation rebuilds its tables from the cores it finds), so nothing is dropped
static int ca_run(ttx_engine *h, const char *who, const double *alpha, const double *g, bool dev)
{
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!alpha || !g) return fail(TTX_EINVAL, "%s: null argument", who);
    if ((rc = cg_check_train(h, who))) return rc;
    const int d = h->d;
    std::vector<CaCore> cs(d);
    long long tot = 0;
    for (int k = 1; k <= d; k++) {
        cs[k - 1] = CaCore{core_dev(h, k), tot, tot, h->rfinal[k - 1], h->n1[k], h->rfinal[k], alpha[k - 1]};
        tot += (long long)core_elems(h, k);
    }
    OpMeta meta(h->meta_host);
    const size_t o_cs = meta.put(cs);
    char *dm = nullptr;
    if ((rc = meta.upload(h, SC_META, &dm))) return rc;
    const double *G = g;
    if (!dev) {
        if ((rc = buf_reserve(h, SC_CGG, sizeof(double) * (size_t)tot))) return rc;
        double *sg = buf<double>(h, SC_CGG);
        for (int k = 0; k < d; k++)                                             // a skipped core's block is not read, not even on the host
            if (cs[k].alpha != 0.0) HIPCHECK(hipMemcpyAsync(sg + cs[k].goff, g + cs[k].goff, sizeof(double) * core_elems(h, k + 1), hipMemcpyHostToDevice, h->stream));
        G = sg;
    }
    hipLaunchKernelGGL(k_cores_axpy, g1((size_t)tot), dim3(256), 0, h->stream, (const CaCore *)(dm + o_cs), d, tot, h->RM, h->P.SS, G);
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_cores_axpy(ttx_engine *h, const double *alpha, const double *g) { return ca_run(h, "ttx_cores_axpy", alpha, g, false); }
extern "C" int ttx_cores_axpy_dev(ttx_engine *h, const double *alpha, const double *g_dev) { return ca_run(h, "ttx_cores_axpy_dev", alpha, g_dev, true); }

// ---- the derivative along a direction in core space (ttx_basis_jvp.h) ------------------------------------------------------------
enum { JVM_TABLE, JVM_CHAIN };             // OpMarks phases of a call, JvLast::ms takes the sums
// in: the coordinates or the caller's phi; v: the packed direction, on the host unless dev; val may be null
static int jv_run(ttx_engine *h, const char *who, BsSrc src, int64_t npts, const double *in, const ttx_basis *basis, const double *v, double *val, double *dval, int32_t mode)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (npts < 0 || (npts > 0 && (!in || !v || !dval || (!tab && !basis)))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    const int d = h->d;
    if (!tab && basis) for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    const JvPlan pl = jv_plan(d, h->n1.data() + 1, h->rfinal.data(), dev_ncu(h), src, !dev, npts, mode, env_chunk("TTX_BASIS_CHUNK", op_chunk_default(h->RM)));
    if (pl.refusal == BS_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.rmax);
    if (pl.refusal == BS_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    h->jv = JvLast();
    h->jv.flops = pl.flops; h->jv.mode = pl.eff;
    if (npts == 0) return TTX_OK;
    EvTrain T;
    if ((rc = ev_train(h, &T))) return rc;
    std::vector<BsMode> M(d);
    if (!tab) {                                                                 // the nodes of the LINEAR modes, one device block
        OpMeta meta(h->meta_host);
        std::vector<size_t> o_nodes(d, 0);
        for (int k = 0; k < d; k++)
            if (basis[k].kind == TTX_BASIS_LINEAR) o_nodes[k] = meta.put(std::vector<double>(basis[k].nodes, basis[k].nodes + h->n1[k + 1]));
        char *dm = nullptr;
        if (!meta.host.empty() && (rc = meta.upload(h, SC_META, &dm))) return rc;
        for (int k = 0; k < d; k++) {
            const ttx_basis &b = basis[k];
            const bool cosk = b.kind == TTX_BASIS_COS;
            M[k] = BsMode{b.kind, b.flags, h->n1[k + 1], cosk ? b.a : 0.0, cosk ? ttx_basis_cos_w(b.a, b.b) : 0.0, cosk ? nullptr : (const double *)(dm + o_nodes[k])};
        }
    }
    if ((rc = buf_reserve(h, {{SC_XA, pl.b_xa}, {SC_XB, pl.b_xb}, {SC_BTAB, pl.b_btab}, {SC_X, pl.b_x}, {SC_OUT, pl.b_out}, {SC_JVV, pl.b_v}}))) return rc;
    double *btab = buf<double>(h, SC_BTAB), *sin_ = buf<double>(h, SC_X), *sout = buf<double>(h, SC_OUT);
    const double *V = v;
    if (!dev) {
        HIPCHECK(hipMemcpyAsync(buf<double>(h, SC_JVV), v, sizeof(double) * pl.vsize, hipMemcpyHostToDevice, h->stream));
        V = buf<double>(h, SC_JVV);
    }
    if (pl.eff == TTX_EVAL_MFMA)
        for (int i = 0; i < d; i++)
            if ((rc = with_tier<true>(pl.step[i].tier, [&](auto mr) { return op_lds_raise(h, reinterpret_cast<const void *>(&k_jv_gemm<decltype(mr)::value>), pl.step[i].lds); }))) return rc;
    OpMarks marks(h->op_ev);
    for (int64_t o = 0; o < npts; o += (int64_t)pl.chunk) {
        const int c = (int)std::min<int64_t>((int64_t)pl.chunk, npts - o);
        const double *cin = in + (size_t)o * pl.row;
        double *cval = val ? val + o : nullptr, *cd = dval + o;
        if (!dev) {
            HIPCHECK(hipMemcpyAsync(sin_, cin, sizeof(double) * (size_t)c * pl.row, hipMemcpyHostToDevice, h->stream));
            cin = sin_; cval = val ? sout : nullptr; cd = sout + pl.chunk;
        }
        double *X = buf<double>(h, SC_XA), *Z = buf<double>(h, SC_XB);
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        for (int i = d - 1; i >= 0; i--) {
            const double *ph = cin + pl.off[i];
            size_t ld = pl.sumn;
            if (!tab) {
                hipLaunchKernelGGL(k_bs_table, g1((size_t)c * M[i].n), dim3(256), 0, h->stream, M[i], (long long)c, cin + i, d, btab);
                if ((rc = marks.mark(h->stream, JVM_TABLE))) return rc;
                ph = btab; ld = (size_t)M[i].n;
            }
            const double *Xin = i == d - 1 ? nullptr : X, *Vi = V + pl.voff[i];
            const int last = i == 0;
            if (pl.eff == TTX_EVAL_EXACT)
                hipLaunchKernelGGL(k_jv_exact, dim3(pl.g_exact(c)), dim3(256), pl.exact_lds, h->stream, T, i, (long long)c, ph, ld, Vi, Xin, Z, pl.ystr, cval, cd, last);
            else
                with_tier<true>(pl.step[i].tier, [&](auto mr) {
                    hipLaunchKernelGGL(k_jv_gemm<decltype(mr)::value>, dim3(pl.g_gemm(i, c), pl.step[i].gy), dim3(256), pl.step[i].lds.bytes, h->stream, T, i, c, ph, ld, Vi, Xin, Z, pl.ystr, cval, cd, last);
                    return 0;
                });
            if ((rc = marks.mark(h->stream, JVM_CHAIN))) return rc;
            std::swap(X, Z);
        }
        if (!dev) {
            if (val) HIPCHECK(hipMemcpyAsync(val + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
            HIPCHECK(hipMemcpyAsync(dval + o, sout + pl.chunk, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
        }
        if (!dev || marks.phase.size() > 4096) {                                // the staging blocks are reused by the next chunk; the event chain stays short
            HIPCHECK(hipStreamSynchronize(h->stream));
            if ((rc = marks.sum(h->jv.ms))) return rc;
        }
    }
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = marks.sum(h->jv.ms))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_basis_jvp_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, const double *v, double *val, double *dval, int32_t mode)
{
    return jv_run(h, "ttx_basis_jvp_batch", BS_X_HOST, npts, x, basis, v, val, dval, mode);
}
extern "C" int ttx_basis_jvp_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *v_dev, double *val_dev, double *dval_dev, int32_t mode)
{
    return jv_run(h, "ttx_basis_jvp_batch_dev", BS_X_DEV, npts, x_dev, basis, v_dev, val_dev, dval_dev, mode);
}
extern "C" int ttx_basis_jvp_tab(ttx_engine *h, int64_t npts, const double *phi, const double *v, double *val, double *dval, int32_t mode)
{
    return jv_run(h, "ttx_basis_jvp_tab", BS_TAB_HOST, npts, phi, nullptr, v, val, dval, mode);
}
extern "C" int ttx_basis_jvp_tab_dev(ttx_engine *h, int64_t npts, const double *phi_dev, const double *v_dev, double *val_dev, double *dval_dev, int32_t mode)
{
    return jv_run(h, "ttx_basis_jvp_tab_dev", BS_TAB_DEV, npts, phi_dev, nullptr, v_dev, val_dev, dval_dev, mode);
}
extern "C" int ttx_basis_jvp_last(const ttx_engine *h, double *ms_table, double *ms_chain, double *flops, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_basis_jvp_last: null engine");
    if (ms_table) *ms_table = h->jv.ms[JVM_TABLE];
    if (ms_chain) *ms_chain = h->jv.ms[JVM_CHAIN];
    if (flops) *flops = h->jv.flops;
    if (mode_ran) *mode_ran = h->jv.mode;
    return TTX_OK;
}

// ---- vector operations on packed core-space buffers (ttx_basis_jvp.h) ------------------------------------------------------------
static size_t cores_total(const ttx_engine *h) { size_t t = 0; for (int k = 1; k <= h->d; k++) t += core_elems(h, k); return t; }
// the fixed-order dot product of two device buffers of tot doubles: the segment sums on the device, their sum on the host
static int vec_dot(ttx_engine *h, long long tot, const double *a, const double *b, double *out)
{
    if (int rc = buf_reserve(h, SC_VDP, sizeof(double) * TTX_DOT_SEGS)) return rc;
    double *part = buf<double>(h, SC_VDP), hp[TTX_DOT_SEGS];
    hipLaunchKernelGGL(k_vec_dot, dim3(TTX_DOT_SEGS), dim3(256), 0, h->stream, tot, dot_seg(tot), a, b, part);
    HIPCHECK(hipMemcpyAsync(hp, part, sizeof(hp), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (int k = 0; k < TTX_DOT_SEGS; k++) s = s + hp[k];
    *out = s;
    return TTX_OK;
}
static int cd_run(ttx_engine *h, const char *who, const double *a, const double *b, double *out, bool dev)
{
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!a || !b || !out) return fail(TTX_EINVAL, "%s: null argument", who);
    if ((rc = cg_check_train(h, who))) return rc;
    const size_t tot = cores_total(h);
    if (!dev) {
        if ((rc = buf_reserve(h, SC_VIN, sizeof(double) * 2 * tot))) return rc;
        double *s = buf<double>(h, SC_VIN);
        HIPCHECK(hipMemcpyAsync(s, a, sizeof(double) * tot, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(hipMemcpyAsync(s + tot, b, sizeof(double) * tot, hipMemcpyHostToDevice, h->stream));
        a = s; b = s + tot;
    }
    if ((rc = vec_dot(h, (long long)tot, a, b, out))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_cores_dot(ttx_engine *h, const double *a, const double *b, double *out) { return cd_run(h, "ttx_cores_dot", a, b, out, false); }
extern "C" int ttx_cores_dot_dev(ttx_engine *h, const double *a_dev, const double *b_dev, double *out) { return cd_run(h, "ttx_cores_dot_dev", a_dev, b_dev, out, true); }
extern "C" int ttx_cores_axpby_dev(ttx_engine *h, double alpha, const double *x_dev, double beta, double *y_dev)
{
    const char *who = "ttx_cores_axpby_dev";
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!x_dev || !y_dev) return fail(TTX_EINVAL, "%s: null argument", who);
    if ((rc = cg_check_train(h, who))) return rc;
    const size_t tot = cores_total(h);
    hipLaunchKernelGGL(k_vec_axpby, g1(tot), dim3(256), 0, h->stream, (long long)tot, alpha, x_dev, beta, y_dev);
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
// the cores to (set: from) a packed device buffer, core by core on the shared pack/push helpers; bit for bit
static int cores_copy_dev(ttx_engine *h, const char *who, double *g, bool set, bool dev = true)
{
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!g) return fail(TTX_EINVAL, "%s: null argument", who);
    if ((rc = cg_check_train(h, who))) return rc;
    size_t off = 0;
    double *hg = g;
    if (!dev) {                                                                 // a host caller's buffer goes through the staging block of ttx_cores_axpy
        if ((rc = buf_reserve(h, SC_CGG, sizeof(double) * cores_total(h)))) return rc;
        g = buf<double>(h, SC_CGG);
        if (set) HIPCHECK(hipMemcpyAsync(g, hg, sizeof(double) * cores_total(h), hipMemcpyHostToDevice, h->stream));
    }
    for (int k = 1; k <= h->d; k++) {
        if (set) unpack_core(h, k, g + off, h->rfinal[k - 1], h->rfinal[k]);
        else pack_core(h->stream, h, k, g + off);
        off += core_elems(h, k);
    }
    if (!dev && !set) HIPCHECK(hipMemcpyAsync(hg, g, sizeof(double) * cores_total(h), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_cores_get(ttx_engine *h, double *g) { return cores_copy_dev(h, "ttx_cores_get", g, false, false); }
extern "C" int ttx_cores_set(ttx_engine *h, const double *g) { return cores_copy_dev(h, "ttx_cores_set", const_cast<double *>(g), true, false); }
extern "C" int ttx_cores_get_dev(ttx_engine *h, double *g_dev) { return cores_copy_dev(h, "ttx_cores_get_dev", g_dev, false); }
extern "C" int ttx_cores_set_dev(ttx_engine *h, const double *g_dev) { return cores_copy_dev(h, "ttx_cores_set_dev", const_cast<double *>(g_dev), true); }

// ---- the Gauss-Newton solver (ttx_fit_plan.h holds the controller; this is its backend on the device) ----------------------------
enum { FTM_JVP, FTM_CG, FTM_VAL, FTM_VEC };
namespace {
struct FitDev {
    ttx_engine *h; const char *who; BsSrc src; int64_t npts; const double *in; const ttx_basis *basis; const double *y, *w; int mode;
    size_t tot = 0;
    double *vec[FIT_NVEC] = {}, *snap = nullptr, *val = nullptr, *q = nullptr, *c = nullptr;     // q: the residual inside loss(), else J p
    std::vector<double> ones;
    // a vector launch between two marks of the engine's event pool
    template <class F> int timed(F f)
    {
        OpMarks marks(h->op_ev);
        int rc;
        if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
        if ((rc = f())) return rc;
        if ((rc = marks.mark(h->stream, FTM_VEC))) return rc;
        HIPCHECK(hipStreamSynchronize(h->stream));
        return marks.sum(h->fit.ms);
    }
    int loss(double *l)
    {
        int rc = bs_run(h, who, src, npts, in, basis, val, mode);
        if (rc) return rc;
        h->fit.ms[FTM_VAL] += h->bs.ms[BSM_TABLE] + h->bs.ms[BSM_CHAIN];
        double s = 0.0;
        if ((rc = timed([&] {
                hipLaunchKernelGGL(k_fit_residual, g1((size_t)npts), dim3(256), 0, h->stream, (long long)npts, val, y, w, q, c);
                return vec_dot(h, (long long)npts, c, q, &s);
            }))) return rc;
        *l = 0.5 * s;
        return TTX_OK;
    }
    int core_grad(int from_q, int dst)
    {
        const double *cw = c;
        int rc;
        if (from_q) {
            if (!w) cw = q;
            else if ((rc = timed([&] { hipLaunchKernelGGL(k_fit_weigh, g1((size_t)npts), dim3(256), 0, h->stream, (long long)npts, w, q, c); return 0; }))) return rc;
        }
        if ((rc = cg_run(h, who, src, npts, in, basis, cw, nullptr, vec[dst], 0, mode))) return rc;
        h->fit.n_cg++;
        for (int k = 0; k < 4; k++) h->fit.ms[FTM_CG] += h->cg.ms[k];
        return TTX_OK;
    }
    int jvp(int v)
    {
        int rc = jv_run(h, who, src, npts, in, basis, vec[v], nullptr, q, mode);
        if (rc) return rc;
        h->fit.n_jvp++; h->fit.mode = h->jv.mode;
        h->fit.ms[FTM_JVP] += h->jv.ms[JVM_TABLE] + h->jv.ms[JVM_CHAIN];
        return TTX_OK;
    }
    int dot(int a, int b, double *s) { return timed([&] { return vec_dot(h, (long long)tot, vec[a], vec[b], s); }); }
    int axpby(double al, int x, double be, int yv)
    {
        return timed([&] { hipLaunchKernelGGL(k_vec_axpby, g1(tot), dim3(256), 0, h->stream, (long long)tot, al, vec[x], be, vec[yv]); return 0; });
    }
    int zero(int v) { return timed([&] { HIPCHECK(hipMemsetAsync(vec[v], 0, sizeof(double) * tot, h->stream)); return 0; }); }
    int copy(int dst, int s) { return timed([&] { HIPCHECK(hipMemcpyAsync(vec[dst], vec[s], sizeof(double) * tot, hipMemcpyDeviceToDevice, h->stream)); return 0; }); }
    int snapshot() { return timed([&] { return cores_copy_dev(h, who, snap, false); }); }
    int restore() { return timed([&] { return cores_copy_dev(h, who, snap, true); }); }
    int apply(int s) { return timed([&] { return ca_run(h, who, ones.data(), vec[s], true); }); }
};
}
static int fit_run_dev(ttx_engine *h, const char *who, BsSrc src, int64_t npts, const double *in, const ttx_basis *basis, const double *y, const double *w,
                       const ttx_fit_opts *opts, double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result)
{
    const bool tab = src == BS_TAB_HOST || src == BS_TAB_DEV, dev = src == BS_X_DEV || src == BS_TAB_DEV;
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!opts || npts < 1 || !in || !y || (!tab && !basis)) return fail(TTX_EINVAL, "%s: null argument or npts < 1", who);
    if (const char *bad = fit_opts_problem(*opts)) return fail(TTX_EINVAL, "%s: %s", who, bad);
    if ((rc = cg_check_train(h, who))) return rc;
    const int d = h->d;
    if (!tab) for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    if (!dev && w) for (int64_t p = 0; p < npts; p++) if (!(w[p] >= 0.0) || !std::isfinite(w[p])) return fail(TTX_EINVAL, "%s: w[%lld] is negative or not finite", who, (long long)p);
    size_t row = (size_t)d;
    double work = 0.0;
    if (tab) { row = 0; for (int k = 1; k <= d; k++) row += (size_t)h->n1[k]; }
    for (int k = 1; k <= d; k++) work += (double)core_elems(h, k);
    FitDev b{h, who, tab ? BS_TAB_DEV : BS_X_DEV, npts, in, basis, y, w, op_mode_eff(opts->mode, 6.0 * (double)npts * work, TTX_JV_AUTO_FLOPS)};
    b.tot = cores_total(h);
    b.ones.assign(d, 1.0);
    // the work vectors g, s, r, p, Ap and the snapshot; the three point vectors, then what a host caller's arrays are uploaded into, once
    const size_t np = (size_t)npts, nin = dev ? 0 : np * row + np + (w ? np : 0);
    if ((rc = buf_reserve(h, {{SC_FITV, sizeof(double) * (FIT_NVEC + 1) * b.tot}, {SC_FITP, sizeof(double) * (3 * np + nin)}}))) return rc;
    double *fv = buf<double>(h, SC_FITV), *fp = buf<double>(h, SC_FITP);
    for (int k = 0; k < FIT_NVEC; k++) b.vec[k] = fv + (size_t)k * b.tot;
    b.snap = fv + (size_t)FIT_NVEC * b.tot;
    b.val = fp; b.q = fp + np; b.c = fp + 2 * np;
    if (!dev) {
        double *ui = fp + 3 * np, *uy = ui + np * row, *uw = uy + np;
        HIPCHECK(hipMemcpyAsync(ui, in, sizeof(double) * np * row, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(hipMemcpyAsync(uy, y, sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
        if (w) HIPCHECK(hipMemcpyAsync(uw, w, sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        b.in = ui; b.y = uy; b.w = w ? uw : nullptr;
    }
    h->fit = FitLast();
    h->fit.mode = b.mode;
    FitHistory hist;
    hist.loss = loss; hist.lambda = lambda; hist.cg_iters = cg_iters; hist.accepted = accepted;
    return fit_run(b, *opts, hist, result);
}
extern "C" int ttx_basis_fit_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, const double *y, const double *w, const ttx_fit_opts *opts,
                                   double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result)
{
    return fit_run_dev(h, "ttx_basis_fit_batch", BS_X_HOST, npts, x, basis, y, w, opts, loss, lambda, cg_iters, accepted, result);
}
extern "C" int ttx_basis_fit_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *y_dev, const double *w_dev, const ttx_fit_opts *opts,
                                       double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result)
{
    return fit_run_dev(h, "ttx_basis_fit_batch_dev", BS_X_DEV, npts, x_dev, basis, y_dev, w_dev, opts, loss, lambda, cg_iters, accepted, result);
}
extern "C" int ttx_basis_fit_tab(ttx_engine *h, int64_t npts, const double *phi, const double *y, const double *w, const ttx_fit_opts *opts,
                                 double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result)
{
    return fit_run_dev(h, "ttx_basis_fit_tab", BS_TAB_HOST, npts, phi, nullptr, y, w, opts, loss, lambda, cg_iters, accepted, result);
}
extern "C" int ttx_basis_fit_tab_dev(ttx_engine *h, int64_t npts, const double *phi_dev, const double *y_dev, const double *w_dev, const ttx_fit_opts *opts,
                                     double *loss, double *lambda, int32_t *cg_iters, int32_t *accepted, ttx_fit_result *result)
{
    return fit_run_dev(h, "ttx_basis_fit_tab_dev", BS_TAB_DEV, npts, phi_dev, nullptr, y_dev, w_dev, opts, loss, lambda, cg_iters, accepted, result);
}
extern "C" int ttx_basis_fit_last(const ttx_engine *h, double *ms_jvp, double *ms_core_grad, double *ms_value, double *ms_vector, int64_t *n_jvp, int64_t *n_core_grad, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_basis_fit_last: null engine");
    if (ms_jvp) *ms_jvp = h->fit.ms[FTM_JVP];
    if (ms_core_grad) *ms_core_grad = h->fit.ms[FTM_CG];
    if (ms_value) *ms_value = h->fit.ms[FTM_VAL];
    if (ms_vector) *ms_vector = h->fit.ms[FTM_VEC];
    if (n_jvp) *n_jvp = h->fit.n_jvp;
    if (n_core_grad) *n_core_grad = h->fit.n_cg;
    if (mode_ran) *mode_ran = h->fit.mode;
    return TTX_OK;
}

// ---- the normaliser of the squared density and its gradient (ttx_sq_norm.h) ------------------------------------------------------
enum { SQM_RIGHT, SQM_LEFT, SQM_ASM };
// what ttx_sq_lognorm_grad refuses of md, mo, gvol, coef, accumulate and mode, asked before anything is touched
static int sqn_check(ttx_engine *h, const char *who, const double *const *md, const double *const *mo, double gvol, double coef, int32_t accumulate, int32_t mode)
{
    if (!md) return fail(TTX_EINVAL, "%s: null md", who);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    if (accumulate != 0 && accumulate != 1) return fail(TTX_EINVAL, "%s: accumulate is 0 or 1 (got %d)", who, accumulate);
    if (!(gvol >= 0.0) || !std::isfinite(gvol)) return fail(TTX_EINVAL, "%s: gvol is negative or not finite", who);
    if (!std::isfinite(coef)) return fail(TTX_EINVAL, "%s: coef is not finite", who);
    for (int k = 1; k <= h->d; k++) {
        if (!md[k - 1]) return fail(TTX_EINVAL, "%s: null md[%d]", who, k - 1);
        for (int i = 0; i < h->n1[k]; i++) if (!std::isfinite(md[k - 1][i])) return fail(TTX_EINVAL, "%s: md[%d][%d] is not finite", who, k - 1, i);
        if (mo && mo[k - 1]) for (int i = 0; i + 1 < h->n1[k]; i++) if (!std::isfinite(mo[k - 1][i])) return fail(TTX_EINVAL, "%s: mo[%d][%d] is not finite", who, k - 1, i);
    }
    return TTX_OK;
}
// g: the packed gradient, on the host unless dev; z_mant, z_exp, logz may be null
static int sqn_run(ttx_engine *h, const char *who, const double *const *md, const double *const *mo, double gvol, double coef, double *g, int32_t accumulate, int32_t mode,
                   bool dev, double *z_mant, int64_t *z_exp, double *logz)
{
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (!g) return fail(TTX_EINVAL, "%s: null argument", who);
    if ((rc = cg_check_train(h, who)) || (rc = sqn_check(h, who, md, mo, gvol, coef, accumulate, mode))) return rc;
    const int d = h->d;
    const std::vector<int32_t> &r = h->rfinal;
    const SqnPlan pl = sqn_plan(d, h->n1.data() + 1, r.data(), !dev, mode);
    if (pl.refusal == BS_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.rmax);
    if (pl.refusal == BS_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    h->sqn = SqnLast();
    h->sqn.flops = pl.flops; h->sqn.mode = pl.eff;
    // the diagonals and the off-diagonals of all modes, one device block each; a mode without an off-diagonal gets a null pointer
    std::vector<double> hd(pl.nsum), ho(pl.nsum, 0.0);
    for (int k = 0; k < d; k++) {
        std::copy(md[k], md[k] + h->n1[k + 1], hd.begin() + pl.noff[k]);
        if (mo && mo[k] && h->n1[k + 1] > 1) std::copy(mo[k], mo[k] + h->n1[k + 1] - 1, ho.begin() + pl.noff[k]);
    }
    OpMeta meta(h->meta_host);
    const size_t o_d = meta.put(hd), o_o = meta.put(ho);
    char *dm = nullptr;
    if ((rc = meta.upload(h, SC_META, &dm))) return rc;
    const double *Dd = (const double *)(dm + o_d), *Do = (const double *)(dm + o_o);
    if ((rc = buf_reserve(h, {{SC_SQNW, pl.b_w}, {SC_SQNP, pl.b_pr + pl.b_pl + pl.b_ex}, {SC_SQNY, pl.b_y + pl.b_part}, {SC_CGG, pl.b_g}}))) return rc;
    double *W = buf<double>(h, SC_SQNW), *PR = buf<double>(h, SC_SQNP), *PL[2] = {PR + pl.proff[d + 1], PR + pl.proff[d + 1] + (size_t)pl.rmax * pl.rmax};
    double *Y = buf<double>(h, SC_SQNY), *Part = Y + pl.b_y / sizeof(double);
    int *eL = (int *)(PL[1] + (size_t)pl.rmax * pl.rmax), *eR = eL + d + 1;
    const int RM = h->RM;
    const size_t SS = h->P.SS;
    OpMarks marks(h->op_ev);
    if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
    hipLaunchKernelGGL(k_sqn_init, dim3(1), dim3(64), 0, h->stream, PL[0], PR + pl.proff[d], eL, eR + d);
    for (int k = d; k >= 2; k--) {                                              // right chain: PR_(k-1) from PR_k
        const int r0 = r[k - 1], n = h->n1[k], r1 = r[k];
        const double *U = core_dev(h, k), *mdk = Dd + pl.noff[k - 1], *mok = (mo && mo[k - 1]) ? Do + pl.noff[k - 1] : nullptr;
        double *Pn = PR + pl.proff[k - 1];
        hipLaunchKernelGGL(k_sqn_w, dim3((unsigned)(n * r0)), dim3(128), 0, h->stream, U, RM, SS, (size_t)1, r1, n, mdk, mok, (const double *)(PR + pl.proff[k]), Y);
        hipLaunchKernelGGL(k_sqn_p, dim3((r0 + 15) / 16, (r0 + 15) / 16, n), dim3(256), 0, h->stream, U, RM, SS, (size_t)1, r1, r0, (const double *)Y, n, Part);
        hipLaunchKernelGGL(k_sqn_pow2, dim3(1), dim3(1024), 0, h->stream, r0 * r0, n, (const double *)Part, Pn, (const int *)(eR + k), eR + k - 1);
    }
    if ((rc = marks.mark(h->stream, SQM_RIGHT))) return rc;
    for (int k = 1; k <= d; k++) {                                              // left chain: W_k and PL_k from PL_(k-1)
        const int r0 = r[k - 1], n = h->n1[k], r1 = r[k];
        const double *U = core_dev(h, k), *mdk = Dd + pl.noff[k - 1], *mok = (mo && mo[k - 1]) ? Do + pl.noff[k - 1] : nullptr;
        double *Wk = W + pl.goff[k - 1], *Pn = PL[k & 1];
        hipLaunchKernelGGL(k_sqn_w, dim3((unsigned)(n * r1)), dim3(128), 0, h->stream, U, RM, (size_t)1, SS, r0, n, mdk, mok, (const double *)PL[(k - 1) & 1], Wk);
        hipLaunchKernelGGL(k_sqn_p, dim3((r1 + 15) / 16, (r1 + 15) / 16, n), dim3(256), 0, h->stream, U, RM, (size_t)1, SS, r0, r1, (const double *)Wk, n, Part);
        hipLaunchKernelGGL(k_sqn_pow2, dim3(1), dim3(1024), 0, h->stream, r1 * r1, n, (const double *)Part, Pn, (const int *)(eL + k - 1), eL + k);
    }
    if ((rc = marks.mark(h->stream, SQM_LEFT))) return rc;
    double zm = 0.0;
    std::vector<int> he(2 * (size_t)(d + 1));
    HIPCHECK(hipMemcpyAsync(&zm, PL[d & 1], sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(he.data(), eL, sizeof(int) * he.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    const long long ze = he[d];
    if (z_mant) *z_mant = zm;
    if (z_exp) *z_exp = ze;
    if (logz) *logz = sqn_logz(zm, ze, gvol);
    // the assembly: every core in one launch
    const bool mfma = pl.eff == TTX_EVAL_MFMA;
    double *G = dev ? g : buf<double>(h, SC_CGG);
    if (!dev && accumulate) HIPCHECK(hipMemcpyAsync(G, g, sizeof(double) * pl.gsize, hipMemcpyHostToDevice, h->stream));
    std::vector<SqnCore> cs(d);
    for (int k = 1; k <= d; k++)
        cs[k - 1] = SqnCore{W + pl.goff[k - 1], PR + pl.proff[k], G + pl.goff[k - 1], mfma ? pl.first_wg[k - 1] : pl.first_e[k - 1], r[k - 1], h->n1[k], r[k], 0,
                            sqn_scale(zm, ze, gvol, coef, he[k - 1], he[(size_t)(d + 1) + k])};
    OpMeta meta2(h->meta_host);
    const size_t o_cs = meta2.put(cs);
    if ((rc = meta2.upload(h, SC_META, &dm))) return rc;
    const SqnCore *dcs = (const SqnCore *)(dm + o_cs);
    if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
    if (!mfma)
        hipLaunchKernelGGL((k_sqn_asm<false, 1>), dim3(pl.grid_exact), dim3(256), 0, h->stream, dcs, d, (long long)pl.gsize, (int)accumulate);
    else
        with_tier(pl.tier, [&](auto mr) {
            hipLaunchKernelGGL((k_sqn_asm<true, decltype(mr)::value>), dim3((unsigned)pl.tot_wg), dim3(256), 0, h->stream, dcs, d, (long long)pl.gsize, (int)accumulate);
            return 0;
        });
    if ((rc = marks.mark(h->stream, SQM_ASM))) return rc;
    if (!dev) HIPCHECK(hipMemcpyAsync(g, G, sizeof(double) * pl.gsize, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = marks.sum(h->sqn.ms))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_sq_lognorm_grad(ttx_engine *h, const double *const *md, const double *const *mo, double gvol, double coef, double *g, int32_t accumulate, int32_t mode,
                                   double *z_mant, int64_t *z_exp, double *logz)
{
    return sqn_run(h, "ttx_sq_lognorm_grad", md, mo, gvol, coef, g, accumulate, mode, false, z_mant, z_exp, logz);
}
extern "C" int ttx_sq_lognorm_grad_dev(ttx_engine *h, const double *const *md, const double *const *mo, double gvol, double coef, double *g_dev, int32_t accumulate, int32_t mode,
                                       double *z_mant, int64_t *z_exp, double *logz)
{
    return sqn_run(h, "ttx_sq_lognorm_grad_dev", md, mo, gvol, coef, g_dev, accumulate, mode, true, z_mant, z_exp, logz);
}
extern "C" int ttx_sq_lognorm_grad_last(const ttx_engine *h, double *ms_right, double *ms_left, double *ms_asm, double *flops, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_sq_lognorm_grad_last: null engine");
    if (ms_right) *ms_right = h->sqn.ms[SQM_RIGHT];
    if (ms_left) *ms_left = h->sqn.ms[SQM_LEFT];
    if (ms_asm) *ms_asm = h->sqn.ms[SQM_ASM];
    if (flops) *flops = h->sqn.flops;
    if (mode_ran) *mode_ran = h->sqn.mode;
    return TTX_OK;
}
// the negative log-likelihood of the squared density at weighted points and its gradient: the value chain, the point kernel, J^T c,
// then the normaliser's term onto it.  val comes from a value chain of its own: c depends on val, and the core gradient's backward
// pass forms val only together with the states that its forward pass, which needs c, consumes chunk by chunk
static int nll_run(ttx_engine *h, const char *who, bool dev, int64_t npts, const double *x, const ttx_basis *basis, const double *w, double gamma,
                   const double *const *md, const double *const *mo, double gvol, int32_t mode, double *nll, double *logz, double *val, double *g)
{
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if (npts < 0 || !g || !nll || !basis || (npts > 0 && !x)) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    if ((rc = cg_check_train(h, who)) || (rc = sqn_check(h, who, md, mo, gvol, 1.0, 0, mode))) return rc;
    if (!(gamma >= 0.0) || !std::isfinite(gamma)) return fail(TTX_EINVAL, "%s: gamma is negative or not finite", who);
    const int d = h->d;
    for (int k = 1; k <= d; k++) if ((rc = bs_check_one(who, k, basis[k - 1], h->n1[k]))) return rc;
    if (!dev && w) for (int64_t p = 0; p < npts; p++) if (!(w[p] >= 0.0) || !std::isfinite(w[p])) return fail(TTX_EINVAL, "%s: w[%lld] is negative or not finite", who, (long long)p);
    const size_t np = (size_t)npts, tot = cores_total(h), nin = dev ? 0 : np * d + (w ? np : 0);
    if ((rc = buf_reserve(h, {{SC_SQNPT, sizeof(double) * (5 * np + nin + 1)}, {SC_CGG, dev ? 0 : sizeof(double) * tot}}))) return rc;
    double *pv = buf<double>(h, SC_SQNPT), *dval = pv, *c = pv + np, *lt = pv + 2 * np, *wv = pv + 3 * np, *one = pv + 4 * np;
    double *G = dev ? g : buf<double>(h, SC_CGG);
    if (dev && val) dval = val;
    if (!dev && npts > 0) {
        double *ux = pv + 5 * np, *uw = ux + np * d;
        HIPCHECK(hipMemcpyAsync(ux, x, sizeof(double) * np * d, hipMemcpyHostToDevice, h->stream));
        if (w) HIPCHECK(hipMemcpyAsync(uw, w, sizeof(double) * np, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
        x = ux; w = w ? uw : nullptr;
    }
    double s1 = 0.0, wsum = 0.0;
    if (npts > 0) {
        if ((rc = bs_run(h, who, BS_X_DEV, npts, x, basis, dval, mode))) return rc;
        hipLaunchKernelGGL(k_sqn_points, g1(np), dim3(256), 0, h->stream, (long long)npts, (const double *)dval, w, gamma, c, lt, wv, one);
        if ((rc = vec_dot(h, (long long)npts, wv, lt, &s1)) || (rc = vec_dot(h, (long long)npts, wv, one, &wsum))) return rc;
    }
    if ((rc = cg_run(h, who, BS_X_DEV, npts, x, basis, c, nullptr, G, 0, mode))) return rc;
    double lz = 0.0;
    if ((rc = sqn_run(h, who, md, mo, gvol, wsum, G, 1, mode, true, nullptr, nullptr, &lz))) return rc;
    *nll = -s1 + wsum * lz;
    if (logz) *logz = lz;
    if (!dev) {
        if (val && npts > 0) HIPCHECK(hipMemcpyAsync(val, dval, sizeof(double) * np, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipMemcpyAsync(g, G, sizeof(double) * tot, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
extern "C" int ttx_sq_nll_batch(ttx_engine *h, int64_t npts, const double *x, const ttx_basis *basis, const double *w, double gamma, const double *const *md, const double *const *mo,
                                double gvol, int32_t mode, double *nll, double *logz, double *val, double *g)
{
    return nll_run(h, "ttx_sq_nll_batch", false, npts, x, basis, w, gamma, md, mo, gvol, mode, nll, logz, val, g);
}
extern "C" int ttx_sq_nll_batch_dev(ttx_engine *h, int64_t npts, const double *x_dev, const ttx_basis *basis, const double *w_dev, double gamma, const double *const *md, const double *const *mo,
                                    double gvol, int32_t mode, double *nll, double *logz, double *val_dev, double *g_dev)
{
    return nll_run(h, "ttx_sq_nll_batch_dev", true, npts, x_dev, basis, w_dev, gamma, md, mo, gvol, mode, nll, logz, val_dev, g_dev);
}

// ---- moments and reduced density matrices of the squared density (ttx_sq_moments.h) ----------------------------------------------
enum { SQT_CHAINS, SQT_BAND, SQT_CARRY, SQT_CLOSE };
// a non-finite entry of an optional observable (rows that are null are not looked at; an off-diagonal counts only where its diagonal is given)
static int sqm_check_rows(ttx_engine *h, const char *who, const char *nd, const char *no, const double *const *dg, const double *const *of)
{
    if (!dg) return TTX_OK;
    for (int k = 1; k <= h->d; k++) {
        if (!dg[k - 1]) continue;
        for (int i = 0; i < h->n1[k]; i++) if (!std::isfinite(dg[k - 1][i])) return fail(TTX_EINVAL, "%s: %s[%d][%d] is not finite", who, nd, k - 1, i);
        if (of && of[k - 1]) for (int i = 0; i + 1 < h->n1[k]; i++) if (!std::isfinite(of[k - 1][i])) return fail(TTX_EINVAL, "%s: %s[%d][%d] is not finite", who, no, k - 1, i);
    }
    return TTX_OK;
}
extern "C" int ttx_sq_moments(ttx_engine *h, const double *const *md, const double *const *mo, const double *const *ad, const double *const *ao,
                              const double *const *a2d, const double *const *a2o, int32_t mode, double *z_mant, int64_t *z_exp, double *bd, double *bo, double *m1, double *c2)
{
    const char *who = "ttx_sq_moments";
    int rc = tt_prepare(h, who);
    if (rc) return rc;
    if ((rc = cg_check_train(h, who)) || (rc = sqn_check(h, who, md, mo, 0.0, 1.0, 0, mode))) return rc;
    if ((rc = sqm_check_rows(h, who, "ad", "ao", ad, ao)) || (rc = sqm_check_rows(h, who, "a2d", "a2o", a2d, a2o))) return rc;
    const int d = h->d;
    const std::vector<int32_t> &r = h->rfinal;
    const bool want_band = bd && bo, want_out = m1 || c2, want_mom = want_out && ad;
    std::vector<unsigned char> selected(d, 0);
    if (ad) for (int k = 0; k < d; k++) selected[k] = ad[k] != nullptr;
    double auto_flops = TTX_SQM_AUTO_FLOPS;
    if (const char *e = getenv("TTX_SQM_AUTO_FLOPS")) { const double v = atof(e); if (v > 0.0) auto_flops = v; }
    const SqmPlan pl = sqm_plan(d, h->n1.data() + 1, r.data(), selected.data(), want_band, want_mom, z_mant || z_exp || want_out, mode, env_int("TTX_SQM_BATCH", 0), auto_flops);
    if (pl.refusal == SQM_RANK) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, pl.rmax);
    if (pl.refusal == SQM_BOUNDARY) return fail(TTX_EINVAL, "%s: boundary ranks are not 1", who);
    if (pl.refusal == SQM_NOTHING) return fail(TTX_EINVAL, "%s: every output is null", who);
    h->sqm = SqmLast();
    h->sqm.flops = pl.flops; h->sqm.mode = pl.eff; h->sqm.steps = pl.steps;
    const int nsel = (int)pl.sel.size();
    const bool mfma = pl.eff == TTX_EVAL_MFMA;
    // the rows of M, A and A2, one device block each; a row that is not given stays 0.0 and is never read
    std::vector<double> rows[6];
    const double *const *src[6] = {md, mo, ad, ao, a2d, a2o};
    for (int x = 0; x < 6; x++) {
        rows[x].assign(pl.nsum, 0.0);
        if (!src[x]) continue;
        for (int k = 0; k < d; k++) {
            const int cnt = (x & 1) ? h->n1[k + 1] - 1 : h->n1[k + 1];
            if (src[x][k] && cnt > 0) std::copy(src[x][k], src[x][k] + cnt, rows[x].begin() + pl.noff[k]);
        }
    }
    OpMeta meta(h->meta_host);
    size_t off[6];
    for (int x = 0; x < 6; x++) off[x] = meta.put(rows[x]);
    char *dm = nullptr;
    if ((rc = meta.upload(h, SC_META, &dm))) return rc;
    auto row = [&](int x, int k) -> const double * { return (src[x] && src[x][k]) ? (const double *)(dm + off[x]) + pl.noff[k] : nullptr; };   // k 0-based
    const size_t RR = (size_t)pl.rmax * pl.rmax, npr = pl.proff[d + 1];
    if ((rc = buf_reserve(h, {{SC_SQMP, pl.b_pr + pl.b_pl + pl.b_ra + pl.b_band + pl.b_dots + pl.b_ex}, {SC_SQNY, pl.b_y + pl.b_part}, {SC_SQMC, nsel > 1 ? pl.b_carry : 0},
                              {SC_SQMW, pl.b_w + pl.b_cpart}}))) return rc;
    double *PR = buf<double>(h, SC_SQMP), *PLs = PR + npr, *RA = PLs + npr, *RA2 = RA + RR, *band = RA2 + RR, *dots = band + pl.b_band / sizeof(double);
    int *eL = (int *)(dots + std::max<size_t>(1, pl.ndots)), *eR = eL + d + 1, *edots = eR + d + 1;
    double *Y = buf<double>(h, SC_SQNY), *Y2 = Y + pl.b_y / (2 * sizeof(double)), *Part = Y + pl.b_y / sizeof(double);
    double *Cc[2] = {buf<double>(h, SC_SQMC), buf<double>(h, SC_SQMC) + (size_t)pl.members * RR};
    int *ce = (int *)(Cc[1] + (size_t)pl.members * RR);
    double *Wb = buf<double>(h, SC_SQMW), *CPart = Wb + pl.b_w / sizeof(double);
    const int RM = h->RM;
    const size_t SS = h->P.SS;
    OpMarks marks(h->op_ev);
    if ((rc = marks.mark(h->stream, OpMarks::DISCARD))) return rc;
    // the chains of ttx_sq_lognorm_grad, launch for launch; every PL_k is kept as every PR_k is
    hipLaunchKernelGGL(k_sqn_init, dim3(1), dim3(64), 0, h->stream, PLs, PR + pl.proff[d], eL, eR + d);
    for (int k = d; k >= 2; k--) {
        const int r0 = r[k - 1], n = h->n1[k], r1 = r[k];
        const double *U = core_dev(h, k);
        hipLaunchKernelGGL(k_sqn_w, dim3((unsigned)(n * r0)), dim3(128), 0, h->stream, U, RM, SS, (size_t)1, r1, n, row(0, k - 1), row(1, k - 1), (const double *)(PR + pl.proff[k]), Y);
        hipLaunchKernelGGL(k_sqn_p, dim3((r0 + 15) / 16, (r0 + 15) / 16, n), dim3(256), 0, h->stream, U, RM, SS, (size_t)1, r1, r0, (const double *)Y, n, Part);
        hipLaunchKernelGGL(k_sqn_pow2, dim3(1), dim3(1024), 0, h->stream, r0 * r0, n, (const double *)Part, PR + pl.proff[k - 1], (const int *)(eR + k), eR + k - 1);
    }
    for (int k = 1; k <= d; k++) {
        const int r0 = r[k - 1], n = h->n1[k], r1 = r[k];
        const double *U = core_dev(h, k);
        hipLaunchKernelGGL(k_sqn_w, dim3((unsigned)(n * r1)), dim3(128), 0, h->stream, U, RM, (size_t)1, SS, r0, n, row(0, k - 1), row(1, k - 1), (const double *)(PLs + pl.proff[k - 1]), Y);
        hipLaunchKernelGGL(k_sqn_p, dim3((r1 + 15) / 16, (r1 + 15) / 16, n), dim3(256), 0, h->stream, U, RM, (size_t)1, SS, r0, r1, (const double *)Y, n, Part);
        hipLaunchKernelGGL(k_sqn_pow2, dim3(1), dim3(1024), 0, h->stream, r1 * r1, n, (const double *)Part, PLs + pl.proff[k], (const int *)(eL + k - 1), eL + k);
    }
    if ((rc = marks.mark(h->stream, SQT_CHAINS))) return rc;
    // the band of every mode's reduced density matrix: the exact kernels in both modes
    if (want_band) {
        for (int k = 1; k <= d; k++) {
            const int r0 = r[k - 1], n = h->n1[k], r1 = r[k];
            const double *U = core_dev(h, k);
            const long long tot = (long long)r0 * n * r1;
            hipLaunchKernelGGL(k_sqm_w, dim3((unsigned)(n * r1), 1), dim3(128), 0, h->stream, U, RM, (size_t)1, SS, r0, n, (const double *)nullptr, (const double *)nullptr,
                               (const double *)(PLs + pl.proff[k - 1]), (size_t)0, Y, (size_t)0);
            hipLaunchKernelGGL(k_sqm_d0, dim3((unsigned)std::min<long long>((tot + 255) / 256, 4096)), dim3(256), 0, h->stream, (long long)r0 * n, r1, (const double *)Y,
                               (const double *)(PR + pl.proff[k]), Y2);
            hipLaunchKernelGGL(k_sqm_band, dim3(n, 2), dim3(128), 0, h->stream, U, RM, SS, r0, n, r1, (const double *)Y2, band + 2 * pl.noff[k - 1]);
        }
        if ((rc = marks.mark(h->stream, SQT_BAND))) return rc;
    }
    // one left step of bc members: P (member stride pst) through mode k with the rows (xd, xo) into dst (compact r1 x r1 each), the
    // exponents ein[c * est] + ex into eout[c]
    auto left_step = [&](int k, const double *xd, const double *xo, const double *P, size_t pst, int bc, double *dst, const int *ein, int est, int *eout) {
        const int r0 = r[k - 1], n = h->n1[k], r1 = r[k];
        const double *U = core_dev(h, k);
        const size_t ost = (size_t)r0 * n * r1;
        if (!mfma) {
            hipLaunchKernelGGL(k_sqm_w, dim3((unsigned)(n * r1), bc), dim3(128), 0, h->stream, U, RM, (size_t)1, SS, r0, n, xd, xo, P, pst, Wb, ost);
            hipLaunchKernelGGL(k_sqm_p, dim3((r1 + 15) / 16, (r1 + 15) / 16, n * bc), dim3(256), 0, h->stream, U, RM, (size_t)1, SS, r0, r1, (const double *)Wb, ost, n, CPart);
            hipLaunchKernelGGL(k_sqm_pow2, dim3(bc), dim3(1024), 0, h->stream, r1 * r1, n, (const double *)CPart, dst, ein, est, eout, 1, 1);
        } else {
            const int nt = (r1 + 15) / 16;
            hipLaunchKernelGGL(k_sqm_w_mfma, dim3((unsigned)((n * r1 + TTX_SQM_TILE_COLS - 1) / TTX_SQM_TILE_COLS), (r0 + 15) / 16, bc), dim3(256), 0, h->stream, U, RM, (size_t)1, SS, r0, n, r1,
                               xd, xo, P, pst, Wb, ost);
            hipLaunchKernelGGL(k_sqm_p_mfma, dim3((nt * nt + 3) / 4, bc), dim3(256), 0, h->stream, U, RM, (size_t)1, SS, r0, r1, (const double *)Wb, ost, n, CPart, (size_t)r1 * r1);
            hipLaunchKernelGGL(k_sqm_pow2, dim3(bc), dim3(1024), 0, h->stream, r1 * r1, 1, (const double *)CPart, dst, ein, est, eout, 1, 1);
        }
    };
    // the right matrix RA_(j-1): the right step with the rows (xd, xo) from PR_j, the sum alone
    auto right_matrix = [&](int j, const double *xd, const double *xo, double *out) {
        const int r0 = r[j - 1], n = h->n1[j], r1 = r[j];
        const double *U = core_dev(h, j);
        hipLaunchKernelGGL(k_sqn_w, dim3((unsigned)(n * r0)), dim3(128), 0, h->stream, U, RM, SS, (size_t)1, r1, n, xd, xo, (const double *)(PR + pl.proff[j]), Y);
        hipLaunchKernelGGL(k_sqn_p, dim3((r0 + 15) / 16, (r0 + 15) / 16, n), dim3(256), 0, h->stream, U, RM, SS, (size_t)1, r1, r0, (const double *)Y, n, Part);
        hipLaunchKernelGGL(k_sqm_pow2, dim3(1), dim3(1024), 0, h->stream, r0 * r0, n, (const double *)Part, out, (const int *)nullptr, 0, (int *)nullptr, 0, 0);
    };
    std::vector<size_t> doff(nsel + 1, 0);                                      // per selected l: m1's product, the diagonal's, then the pairs below it
    for (int x = 0; x < nsel; x++) doff[x + 1] = doff[x] + 2 + (size_t)x;
    if (nsel) {
        const int smax = pl.sel.back() + 1;                                     // 1-based
        int cnt = 0, cur = 0;
        for (int j = pl.sel[0] + 1; j <= smax; j++) {
            const bool is_sel = selected[j - 1] != 0;
            const int r0 = r[j - 1], r1 = r[j];
            if (is_sel) {
                const size_t o = doff[cnt];
                right_matrix(j, row(2, j - 1), row(3, j - 1), RA);
                hipLaunchKernelGGL(k_sqm_dot, dim3(1), dim3(256), 0, h->stream, r0 * r0, (const double *)(PLs + pl.proff[j - 1]), (size_t)0, (const double *)RA, (const int *)nullptr, dots + o, edots + o);
                if (cnt) hipLaunchKernelGGL(k_sqm_dot, dim3(cnt), dim3(256), 0, h->stream, r0 * r0, (const double *)Cc[cur], (size_t)r0 * r0, (const double *)RA, (const int *)ce, dots + o + 2, edots + o + 2);
                if (row(4, j - 1)) {
                    right_matrix(j, row(4, j - 1), row(5, j - 1), RA2);
                    hipLaunchKernelGGL(k_sqm_dot, dim3(1), dim3(256), 0, h->stream, r0 * r0, (const double *)(PLs + pl.proff[j - 1]), (size_t)0, (const double *)RA2, (const int *)nullptr, dots + o + 1, edots + o + 1);
                }
                if ((rc = marks.mark(h->stream, SQT_CLOSE))) return rc;
            }
            if (j == smax) break;
            for (int c0 = 0; c0 < cnt; c0 += pl.batch) {
                const int bc = std::min(pl.batch, cnt - c0);
                left_step(j, row(0, j - 1), row(1, j - 1), Cc[cur] + (size_t)c0 * r0 * r0, (size_t)r0 * r0, bc, Cc[cur ^ 1] + (size_t)c0 * r1 * r1, ce + c0, 1, ce + c0);
            }
            if (is_sel) {
                left_step(j, row(2, j - 1), row(3, j - 1), PLs + pl.proff[j - 1], 0, 1, Cc[cur ^ 1] + (size_t)cnt * r1 * r1, eL + j - 1, 0, ce + cnt);
                cnt++;
            }
            cur ^= 1;
            if ((rc = marks.mark(h->stream, SQT_CARRY))) return rc;
        }
    }
    double zm = 0.0;
    std::vector<int> he(2 * (size_t)(d + 1)), hed(std::max<size_t>(1, pl.ndots), 0);
    std::vector<double> hdots(std::max<size_t>(1, pl.ndots), 0.0), hband(want_band ? 2 * pl.nsum : 0);
    HIPCHECK(hipMemcpyAsync(&zm, PLs + pl.proff[d], sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(he.data(), eL, sizeof(int) * he.size(), hipMemcpyDeviceToHost, h->stream));
    if (pl.ndots) {
        HIPCHECK(hipMemcpyAsync(hdots.data(), dots, sizeof(double) * pl.ndots, hipMemcpyDeviceToHost, h->stream));
        HIPCHECK(hipMemcpyAsync(hed.data(), edots, sizeof(int) * pl.ndots, hipMemcpyDeviceToHost, h->stream));
    }
    if (want_band) HIPCHECK(hipMemcpyAsync(hband.data(), band, sizeof(double) * hband.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = marks.sum(h->sqm.ms))) return rc;
    HIPCHECK(hipGetLastError());
    // nothing has been written so far; from here on nothing can fail
    const long long ze = he[d];
    const int *heL = he.data(), *heR = he.data() + d + 1;
    if (z_mant) *z_mant = zm;
    if (z_exp) *z_exp = ze;
    if (want_band)
        for (int k = 0; k < d; k++) {
            const int n = h->n1[k + 1];
            const double *b = hband.data() + 2 * pl.noff[k];
            for (int i = 0; i < n; i++) {
                bd[pl.noff[k] + i] = sqm_ratio(b[i], zm, heL[k], heR[k + 1], ze);
                bo[pl.noff[k] + i] = i + 1 < n ? sqm_ratio(b[n + i], zm, heL[k], heR[k + 1], ze) : 0.0;
            }
        }
    if (m1) std::fill(m1, m1 + d, 0.0);
    if (c2) std::fill(c2, c2 + (size_t)d * d, 0.0);
    for (int x = 0; x < nsel; x++) {
        const int l = pl.sel[x];
        const size_t o = doff[x];
        if (m1) m1[l] = sqm_ratio(hdots[o], zm, heL[l], heR[l + 1], ze);
        if (!c2) continue;
        if (a2d && a2d[l]) c2[(size_t)l * d + l] = sqm_ratio(hdots[o + 1], zm, heL[l], heR[l + 1], ze);
        for (int y = 0; y < x; y++) {
            const int k = pl.sel[y];
            c2[(size_t)k * d + l] = c2[(size_t)l * d + k] = sqm_ratio(hdots[o + 2 + y], zm, hed[o + 2 + y], heR[l + 1], ze);
        }
    }
    return TTX_OK;
}
extern "C" int ttx_sq_moments_last(const ttx_engine *h, double *ms_chains, double *ms_band, double *ms_carry, double *ms_close, double *flops, int64_t *steps, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_sq_moments_last: null engine");
    if (ms_chains) *ms_chains = h->sqm.ms[SQT_CHAINS];
    if (ms_band) *ms_band = h->sqm.ms[SQT_BAND];
    if (ms_carry) *ms_carry = h->sqm.ms[SQT_CARRY];
    if (ms_close) *ms_close = h->sqm.ms[SQT_CLOSE];
    if (flops) *flops = h->sqm.flops;
    if (steps) *steps = h->sqm.steps;
    if (mode_ran) *mode_ran = h->sqm.mode;
    return TTX_OK;
}

// ---- the largest elements of the resident train (ttx_topk.h)--------------------------------------------------------------------
namespace {
struct TkWork {                             // where the plan's slots and tables lie on the device
    char *dm = nullptr;                     // SC_META: nI, ifx, cnt, sheet
    size_t o_nI = 0, o_ifx = 0, o_cnt = 0, o_sheet = 0;
    double *Pb = nullptr, *W = nullptr, *Xo = nullptr, *Xn = nullptr;           // the Gram matrices, the W of a Gram step, the states before and after a mode
    tk_u64 *S = nullptr, *st = nullptr, *blk = nullptr;                         // a mode's keys; the selection's words and chunk counts
    unsigned *hist = nullptr;
    int *rec = nullptr, *tind = nullptr, *oind = nullptr;                       // the kept positions [d][K]; the index rows before and after the ordering
    double *tval = nullptr, *oval = nullptr;
};
}
// the tables to the device, every slot reserved once, the outputs cleared, P_0 = [1] and the x of the empty suffix
static int tk_begin(ttx_engine *h, const TkPlan &pl, int K, TkWork &w)
{
    int rc;
    const int d = h->d;
    OpMeta meta(h->meta_host);
    w.o_nI = meta.put(pl.nI); w.o_ifx = meta.put(pl.ifx); w.o_cnt = meta.put(pl.cnt); w.o_sheet = meta.put(pl.sheet);
    if ((rc = meta.upload(h, SC_META, &w.dm)) ||
        (rc = buf_reserve(h, {{SC_KP, pl.b_kp}, {SC_KW, pl.b_kw}, {SC_KS, pl.b_ks}, {SC_KX, pl.b_kx}, {SC_KREC, pl.b_krec}, {SC_KSEL, pl.b_ksel}, {SC_KOUT, pl.b_kout}}))) return rc;
    w.Pb = buf<double>(h, SC_KP); w.W = buf<double>(h, SC_KW); w.Xo = buf<double>(h, SC_KX); w.Xn = w.Xo + (size_t)K * pl.ldx;
    w.S = buf<tk_u64>(h, SC_KS); w.st = buf<tk_u64>(h, SC_KSEL); w.blk = w.st + TKS_WORDS;
    w.hist = (unsigned *)(w.blk + TTX_TK_SHEET / TTX_TK_CHUNK);
    w.rec = buf<int>(h, SC_KREC);
    w.tval = buf<double>(h, SC_KOUT); w.oval = w.tval + K;                      // [tval K][oval K][tind K d][oind K d]
    w.tind = (int *)(w.oval + K); w.oind = w.tind + (size_t)K * d;
    const double one = 1.0;
    HIPCHECK(hipMemsetAsync(w.rec, 0, pl.b_krec, h->stream));
    HIPCHECK(hipMemsetAsync(w.tval, 0, pl.b_kout, h->stream));
    HIPCHECK(hipMemcpyAsync(w.Pb, &one, sizeof one, hipMemcpyHostToDevice, h->stream));     // P_0 = [1]
    HIPCHECK(hipMemcpyAsync(w.Xo, &one, sizeof one, hipMemcpyHostToDevice, h->stream));     // x of the empty suffix
    return TTX_OK;
}
// the Gram chain: P_k for k = 1 .. d-1 (P_(k-1) scores mode k), between TM_GRAM's events
static int tk_gram(ttx_engine *h, const TkPlan &pl, const TkWork &w)
{
    int rc;
    const int d = h->d, ldp = pl.ldx;
    if (d < 2) return TTX_OK;
    OpTimer &t_gram = h->timer[TM_GRAM];
    if ((rc = t_gram.start(h->stream))) return rc;
    for (int k = 0; k + 1 < d; k++) {
        const int r0 = h->rfinal[k], r1 = h->rfinal[k + 1];
        const double *G = core_dev(h, k + 1), *P = w.Pb + (size_t)k * ldp * ldp;
        hipLaunchKernelGGL(k_tk_gram_w, dim3((unsigned)(pl.nI[k] * r1)), dim3(128), 0, h->stream, G, h->RM, h->P.SS, r0, pl.nI[k], pl.ifx[k], P, ldp, w.W);
        hipLaunchKernelGGL(k_tk_gram_p, dim3((r1 + 15) / 16, (r1 + 15) / 16), dim3(256), 0, h->stream, G, h->RM, h->P.SS, r0, r1, pl.nI[k], pl.ifx[k], (const double *)w.W,
                           w.Pb + (size_t)(k + 1) * ldp * ldp, ldp);
    }
    return t_gram.stop(h->stream);
}
// 0-based mode k: its sheet scored (TM_SCORE), the K largest keys selected and their pairs advanced (TM_SELECT), the wait, the times
static int tk_mode(ttx_engine *h, const TkPlan &pl, int K, int k, TkWork &w)
{
    int rc;
    const int d = h->d, ldx = pl.ldx, ldp = pl.ldx, r0 = h->rfinal[k], r1 = h->rfinal[k + 1], C = pl.cnt[k + 1], Cn = pl.cnt[k], first = k == 0, nI = pl.nI[k], ifx = pl.ifx[k];
    const TkStep &s = pl.step[k];
    const long long M = pl.sheet[k];
    const double *G = core_dev(h, k + 1), *P = w.Pb + (size_t)k * ldp * ldp;
    OpTimer &t_score = h->timer[TM_SCORE], &t_sel = h->timer[TM_SELECT];
    if ((rc = t_score.start(h->stream))) return rc;
    if (pl.eff == TTX_EVAL_MFMA) {
        if ((rc = with_tier(s.tier, [&](auto mr) {
                constexpr int MR = decltype(mr)::value;
                if (int rc = op_lds_raise(h, reinterpret_cast<const void *>(k_tk_score_mfma<MR>), s.lds)) return rc;      // rank 113 .. 128: 66560 bytes
                hipLaunchKernelGGL(k_tk_score_mfma<MR>, dim3(s.gx, s.gy), dim3(256), s.lds.bytes, h->stream, G, h->RM, h->P.SS, r0, r1, P, ldp, (const double *)w.Xo, ldx, C, nI, ifx,
                                   s.niper, first, w.S);
                return (int)TTX_OK;
            }))) return rc;
    } else
        hipLaunchKernelGGL(k_tk_score_exact, dim3(s.g_exact), dim3(256), sizeof(double) * 4 * ldx, h->stream, G, h->RM, h->P.SS, r0, r1, P, ldp, (const double *)w.Xo, ldx, C, nI, ifx,
                           first, w.S);
    if ((rc = t_score.stop(h->stream)) || (rc = t_sel.start(h->stream))) return rc;
    // selection: everything is kept, or the K-th largest key by six radix passes from the top (11, 11, 11, 11, 11 and 9 bits)
    hipLaunchKernelGGL(k_tk_selinit, dim3(1), dim3(1024), 0, h->stream, w.st, w.hist, (long long)K, M, s.radix ? 0 : 1, k == d - 1 ? 1 : 0);
    if (s.radix) {
        static const int shifts[6] = {53, 42, 31, 20, 9, 0};
        for (int shift : shifts) {
            const int nbits = shift ? 11 : 9;
            hipLaunchKernelGGL(k_tk_hist, dim3(s.hg), dim3(256), 0, h->stream, (const tk_u64 *)w.S, M, shift, nbits, shift == 53 ? 1 : 0, (const tk_u64 *)w.st, w.hist);
            hipLaunchKernelGGL(k_tk_pick, dim3(1), dim3(1024), 0, h->stream, w.st, w.hist, shift);
        }
    }
    hipLaunchKernelGGL(k_tk_count, dim3(s.nblk), dim3(1024), 0, h->stream, (const tk_u64 *)w.S, M, (const tk_u64 *)w.st, w.blk);
    hipLaunchKernelGGL(k_tk_blkscan, dim3(1), dim3(1024), 0, h->stream, w.blk, s.nblk);
    hipLaunchKernelGGL(k_tk_scatter, dim3(s.nblk), dim3(1024), 0, h->stream, (const tk_u64 *)w.S, M, w.st, (const tk_u64 *)w.blk, w.rec + (size_t)k * K, Cn);
    hipLaunchKernelGGL(k_tk_advance, dim3(s.g_adv), dim3(256), sizeof(double) * 4 * ldx, h->stream, G, h->RM, h->P.SS, r0, r1, k == d - 1 ? 1 : 0,
                       (const int *)(w.rec + (size_t)k * K), Cn, M, nI, ifx, (const double *)w.Xo, w.Xn, ldx);
    if ((rc = t_sel.stop(h->stream))) return rc;
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    double a = 0.0, b = 0.0;
    if ((rc = t_score.ms(&a)) || (rc = t_sel.ms(&b))) return rc;
    h->tk.ms_score += a; h->tk.ms_select += b;
    std::swap(w.Xo, w.Xn);
    return TTX_OK;
}
// the index rows by back-tracking the kept positions, their ordering by `which`, the read-back and the bound
static int tk_finish(ttx_engine *h, const TkPlan &pl, int K, int which, const TkWork &w, int32_t *nfound, int32_t *ind, double *val, double *bound)
{
    const int d = h->d, nf = pl.cnt[0];
    hipLaunchKernelGGL(k_tk_back, dim3((nf + 255) / 256), dim3(256), 0, h->stream, d, K, nf, (const int *)w.rec, (const int *)(w.dm + w.o_nI), (const int *)(w.dm + w.o_ifx),
                       (const int *)(w.dm + w.o_cnt), (const long long *)(w.dm + w.o_sheet), (const double *)w.Xo, pl.ldx, w.tind, w.tval);
    hipLaunchKernelGGL(k_tk_order, dim3((nf + 255) / 256), dim3(256), 0, h->stream, d, nf, which, (const int *)w.tind, (const double *)w.tval, w.oind, w.oval);
    tk_u64 fin[TKS_WORDS];
    HIPCHECK(hipMemcpyAsync(ind, w.oind, sizeof(int) * (size_t)K * d, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(val, w.oval, sizeof(double) * K, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipMemcpyAsync(fin, w.st, sizeof fin, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    HIPCHECK(hipGetLastError());
    *nfound = nf;
    if (fin[TKS_NAN]) *bound = __builtin_nan("");
    else if (!fin[TKS_BOUND]) *bound = 0.0;
    else { const tk_u64 bits = fin[TKS_BOUND] - 1ull; memcpy(bound, &bits, sizeof bits); }
    return d > 1 ? h->timer[TM_GRAM].ms(&h->tk.ms_gram) : TTX_OK;
}
extern "C" int ttx_topk(ttx_engine *h, int32_t K, int32_t which, const int32_t *fixed, int32_t mode, int32_t *nfound, int32_t *ind, double *val, double *bound)
{
    const char *who = "ttx_topk";
    if (!nfound || !ind || !val || !bound) return fail(TTX_EINVAL, "%s: null argument", who);
    if (K < 1 || K > TTX_TK_KMAX) return fail(TTX_EINVAL, "%s: K = %d (1 .. %d expected)", who, K, TTX_TK_KMAX);
    if (which != TTX_TOPK_ABS && which != TTX_TOPK_MAX && which != TTX_TOPK_MIN) return fail(TTX_EINVAL, "%s: unknown which %d", who, which);
    if (!op_mode_known(mode)) return fail(TTX_EINVAL, "%s: unknown mode %d", who, mode);
    int rc = check_train_one_process(h, who);
    if (rc || (rc = sm_check_fixed(h, who, fixed))) return rc;
    const TkPlan pl = tk_plan(h->d, h->n1.data() + 1, h->rfinal.data(), dev_ncu(h), K, fixed, mode);
    if (pl.refused)
        return fail(TTX_EINVAL, "%s: K = %d times the largest mode %d is %lld, the score sheet holds up to %d", who, K, pl.nmax, (long long)K * pl.nmax, TTX_TK_SHEET);
    EvTrain T;                              // not read by the kernels: the call keeps ev_train's rank check and its block in SC_TRAIN
    if ((rc = ev_train(h, &T))) return rc;
    TkWork w;
    h->tk = TkLast{0.0, 0.0, 0.0, pl.flops, pl.eff};
    if ((rc = tk_begin(h, pl, K, w)) || (rc = tk_gram(h, pl, w))) return rc;
    for (int k = h->d - 1; k >= 0; k--) if ((rc = tk_mode(h, pl, K, k, w))) return rc;
    return tk_finish(h, pl, K, which, w, nfound, ind, val, bound);
}
extern "C" int ttx_topk_last(const ttx_engine *h, double *ms_gram, double *ms_score, double *ms_select, double *flops, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "ttx_topk_last: null engine");
    if (ms_gram) *ms_gram = h->tk.ms_gram;
    if (ms_score) *ms_score = h->tk.ms_score;
    if (ms_select) *ms_select = h->tk.ms_select;
    if (flops) *flops = h->tk.flops;
    if (mode_ran) *mode_ran = h->tk.mode;
    return TTX_OK;
}

// ---- samples from the square of the resident train (ttx_sample_sq.h) -----------------------------------------------------------
namespace {
struct SqHead {                             // what sq_head leaves for the draw of ttx_sample_sq and of ttx_sample_sq_real: tables on the device
    double *H = nullptr, *F = nullptr, *g = nullptr;    // SqPlan's H and F tables; g[k]: the defensive term of 0-based mode k in the units of F_k
    const double *w = nullptr;              // the effective weights
    const int *fixed = nullptr;
    const double *sp = nullptr, *nodes = nullptr;       // ttx_sample_sq_real: the superdiagonals beside w (the diagonals), the node block
};
}
// The one left-to-right pass: F_k and H_k by the plan pl for the effective weights eff (mode k at pl.woff[k]) and gw[k] = gamma prod_(j < k) W_j.
// Between TM_HEAD's events; the resident train is only read.  sp and nodes (ttx_sample_sq_real): eff holds the diagonals dg of the modes' bidiagonal
// factors, sp their superdiagonals, and the rows of the QR are dg(i) H_k(a, i, :) + sp(i) H_k(a, i+1, :); nodes is uploaded beside them.
static int sq_head(ttx_engine *h, const SqPlan &pl, const std::vector<double> &eff, const std::vector<int> &fx, const std::vector<double> &gw, SqHead &Q,
                   const std::vector<double> *sp = nullptr, const std::vector<double> *nodes = nullptr)
{
    int rc;
    const int d = h->d;
    const std::vector<int32_t> &r = h->rfinal;
    OpMeta meta(h->meta_host);
    const size_t o_w = meta.put(eff), o_fx = meta.put(fx), o_sp = sp ? meta.put(*sp) : 0, o_nodes = nodes ? meta.put(*nodes) : 0;
    char *dm;
    if ((rc = meta.upload(h, SC_META, &dm)) || (rc = buf_reserve(h, SC_QH, sizeof(double) * pl.hoff[d])) ||
        (rc = buf_reserve(h, SC_QF, sizeof(double) * (pl.foff[d] + (size_t)d + 2)))) return rc;
    Q.w = (const double *)(dm + o_w); Q.fixed = (const int *)(dm + o_fx);
    Q.sp = sp ? (const double *)(dm + o_sp) : nullptr; Q.nodes = nodes ? (const double *)(dm + o_nodes) : nullptr;
    Q.H = buf<double>(h, SC_QH); Q.F = buf<double>(h, SC_QF); Q.g = Q.F + pl.foff[d];
    int *st = (int *)(Q.g + d);
    const TtScratch s(h);
    OpTimer &t_head = h->timer[TM_HEAD];
    if ((rc = t_head.start(h->stream))) return rc;
    hipLaunchKernelGGL(k_sq_init, dim3(1), dim3(64), 0, h->stream, Q.F, Q.g, st, gw[0]);      // F_0 = [1], no exponent yet
    for (int k = 1; k <= d; k++) {
        const int r0 = r[k - 1], n = h->n1[k], r1 = r[k], r1p = (r1 + 3) & ~3, l = pl.l[k - 1], mm = l * n;
        pack_core(h->stream, h, k, h->Wb);
        gemm(h, l, n * r1, r0, Q.F + pl.foff[k - 1], l, h->Wb, r0, h->Wc, l);
        hipLaunchKernelGGL(k_sq_split, g1((size_t)mm * r1p), dim3(256), 0, h->stream, (const double *)h->Wc, l, n, r1, r1p, Q.w + pl.woff[k - 1],
                           Q.sp ? Q.sp + pl.woff[k - 1] : (const double *)nullptr, Q.H + pl.hoff[k - 1], k < d ? h->Wa : (double *)nullptr);
        if (k == d) break;
        const double *R = h->Wa;
        int ldr = mm;
        if (mm > r1) { if ((rc = qr(h, mm, r1, h->Wa, s.Rm, s.tau))) return rc; R = s.Rm; ldr = r1; }
        hipLaunchKernelGGL(k_sq_pow2, dim3(1), dim3(1024), 0, h->stream, pl.l[k], r1, R, ldr, Q.F + pl.foff[k], st, gw[k], Q.g + k);
    }
    if ((rc = t_head.stop(h->stream))) return rc;
    HIPCHECK(hipGetLastError());
    return TTX_OK;
}
namespace {
// What tells the two squared samplers apart beside their launches and outputs.  which: SMP_SQ, SMP_SQ_REAL or SMP_ROS_SQ_REAL (the way back shares the real sampler's); sheets: the sheets of
// chunk x nmax doubles in SC_QS; tile: what the 16 indices of an index tile of the MFMA rows advance by (16, or 15: every cell has both
// of its nodes in one tile); state: the bytes a sample keeps in SC_QX between the launches, behind the two state buffers
struct SqKind { int which, sheets, tile; size_t state; };
// one mode of one chunk as sq_frame hands it to the callers' launches
struct SqAt {
    int k, r0, r1, n, l, ldx, C, grid;      // the 0-based mode, its ranks, size and the rows l of its table; the chunk's C samples and the grid of a launch with one wave per sample
    int first, last;                        // k == d - 1, k == 0
    const double *Hk, *Xo, *du;             // the mode's table H_k, the states before the step, the chunk's uniforms
    double *Xn, *S, *state;                 // the states after the step, the sheets (sheet doubles each), the samples' own state (chunk of each array)
    size_t sheet, chunk, woff;              // woff: where the mode's weights start in Q's tables
    const SqHead *Q;                        // the head pass's tables
};
template <int KS> struct SqKs { static constexpr int value = KS; };
}
// The frame of ttx_sample_sq and ttx_sample_sq_real behind their own argument checks; fx[k] != 0: mode k is held.  It holds the plan,
// the sheet check, the reset of the sampler's last-call figures, the head pass, the AUTO decision, the work space, the chunk loop
// (sm_chunks) with the rows, pick and step of every mode between the marks, and the readout of the times.  The callers supply:
//   check(pl)          their last argument check, between the rank check and the sheet check
//   head(pl, Q)        their effective weights or factors, and sq_head with them
//   rows_mfma(ks, a, g, tper), rows_exact(a, g)     the rows launch of a drawn mode on the grid g; ks: SqKs<KS>, KS quads of the rank
//   pick_step(a)       the pick and the step launch of a mode
//   count(c, dcnt)     the launch that adds the chunk's failed samples to dcnt
// and out[0 .. nout-1], the outputs (sm_chunks), whose dev their launches read.
template <class Check, class Head, class RowsMfma, class RowsExact, class PickStep, class Count>
static int sq_frame(ttx_engine *h, const char *who, const SqKind &kind, int64_t npts, const double *u, int32_t mode, bool dev, const std::vector<int> &fx, SmStage *out,
                    int nout, Check check, Head head, RowsMfma rows_mfma, RowsExact rows_exact, PickStep pick_step, Count count)
{
    int rc;
    const int d = h->d;
    SqPlan pl;
    sq_plan(d, h->n1.data() + 1, h->rfinal.data(), fx.data(), pl);
    const int rmax = pl.rmax, nmax = pl.nmax;
    if (rmax > 128) return fail(TTX_EINVAL, "%s: ranks up to 128 only (got %d)", who, rmax);
    if ((rc = check(pl))) return rc;
    const size_t chunk = sm_chunk(std::max<int64_t>(npts, 1)), sheet = chunk * nmax;   // at least 1: this check comes before the early return of an empty call
    const long long held_sheets = (long long)kind.sheets * (long long)chunk * nmax;
    if (held_sheets > TTX_SQ_SHEET)
        return fail(TTX_EINVAL, kind.sheets == 1 ? "%s: a chunk of %zu samples times the largest mode %d is %lld, the sheet holds up to %lld (lower TTX_SAMPLE_CHUNK)"
                                                 : "%s: two sheets of a chunk of %zu samples times the largest mode %d are %lld, they hold up to %lld (lower TTX_SAMPLE_CHUNK)",
                    who, chunk, nmax, held_sheets, (long long)TTX_SQ_SHEET);
    SampleLast &last = h->smp[kind.which];
    last = SampleLast();
    if (npts == 0) return TTX_OK;
    if ((rc = tt_prepare(h, who))) return rc;
    SmLoop P = sm_loop(h, npts);
    SqHead Q;
    if ((rc = head(pl, Q))) return rc;
    const double flops = pl.flops * (double)npts;
    // measured for ttx_sample_sq (ttx_sample_sq.h); ttx_sample_sq_real's modes part in the same bracket on the D_64 train (profiles/sample_sq_real_mi355x.txt)
    const int eff_mode = op_mode_eff(mode, flops, TTX_SQ_AUTO_FLOPS);
    last.flops = flops; last.mode = eff_mode;
    const int ldx = (rmax + 3) & ~3, ncu = dev_ncu(h);
    if ((rc = buf_reserve(h, SC_QS, sizeof(double) * kind.sheets * sheet)) || (rc = buf_reserve(h, SC_QX, (sizeof(double) * 2 * (size_t)ldx + kind.state) * chunk)) ||
        (rc = buf_reserve(h, SC_CNT, sizeof(long long)))) return rc;
    double *Xa = buf<double>(h, SC_QX), *Xb = Xa + chunk * ldx;
    P.dcnt = buf<long long>(h, SC_CNT);
    HIPCHECK(hipMemsetAsync(P.dcnt, 0, sizeof(long long), h->stream));
    OpMarks marks(h->op_ev);                // phase 0: between the chunks, 1: rows, 2: picks and steps
    int lrc = TTX_OK;
    double ms_all = 0.0;
    rc = sm_chunks(h, P, npts, u, dev, out, nout,
        [&](size_t c, int grid, const double *du) {
            SqAt a{};
            a.ldx = ldx; a.C = (int)c; a.grid = grid; a.du = du; a.S = buf<double>(h, SC_QS); a.state = Xb + chunk * ldx; a.sheet = sheet; a.chunk = chunk; a.Q = &Q;
            double *Xo = Xa, *Xn = Xb;
            hipLaunchKernelGGL(k_sq_ones, g1(c), dim3(256), 0, h->stream, Xo, ldx, a.C);        // x of the empty suffix
            if (!lrc) lrc = marks.mark(h->stream, 0);
            for (int k = d - 1; k >= 0; k--) {
                a.k = k; a.r0 = h->rfinal[k]; a.r1 = h->rfinal[k + 1]; a.n = h->n1[k + 1]; a.l = pl.l[k]; a.first = k == d - 1 ? 1 : 0; a.last = k == 0 ? 1 : 0;
                a.Hk = Q.H + pl.hoff[k]; a.woff = pl.woff[k]; a.Xo = Xo; a.Xn = Xn;
                if (!fx[k]) {
                    if (eff_mode == TTX_EVAL_MFMA) {
                        const int lap = 16 - kind.tile, by = (a.C + 63) / 64, nt = (a.n - lap + kind.tile - 1) / kind.tile;
                        const int tper = (int)std::max<long long>(1, (long long)nt * by / (4ll * ncu));
                        const dim3 g((nt + tper - 1) / tper, by);
                        with_tier(rank_tier(a.r1), [&](auto mr) { rows_mfma(SqKs<4 * decltype(mr)::value>(), a, g, tper); return 0; });
                    } else rows_exact(a, dim3((unsigned)std::min<long long>(((long long)a.C * a.n + 255) / 256, (long long)ncu * 16)));
                    if (!lrc) lrc = marks.mark(h->stream, 1);
                }
                pick_step(a);
                if (!lrc) lrc = marks.mark(h->stream, 2);
                std::swap(Xo, Xn);
            }
        },
        [&](size_t c) { count(c, P.dcnt); }, &ms_all, &last.failed);
    if (rc || (rc = lrc)) return rc;
    double ms[3] = {0.0, 0.0, 0.0};
    if ((rc = marks.sum(ms))) return rc;
    last.ms_rows = ms[1]; last.ms_pick = ms[2];
    return h->timer[TM_HEAD].ms(&last.ms_head);
}
// the last-call figures of a squared sampler (which) as its _last entry hands them out; any pointer may be null
static int sq_last(const ttx_engine *h, const char *who, int which, double *ms_head, double *ms_rows, double *ms_pick, double *flops, int64_t *nfailed, int32_t *mode_ran)
{
    if (!h) return fail(TTX_EINVAL, "%s: null engine", who);
    const SampleLast &L = h->smp[which];
    if (ms_head) *ms_head = L.ms_head;
    if (ms_rows) *ms_rows = L.ms_rows;
    if (ms_pick) *ms_pick = L.ms_pick;
    if (flops) *flops = L.flops;
    if (nfailed) *nfailed = L.failed;
    if (mode_ran) *mode_ran = L.mode;
    return TTX_OK;
}
// both entries: u, ind, logq, val are host pointers (dev false: staged chunk by chunk) or pointers on the engine's device.  One sheet, index
// tiles of 16, per sample logq and the failure flag (SqState)
static int sq_run(ttx_engine *h, const char *who, int64_t npts, const double *u, const double *w, const int32_t *fixed, double gamma, int32_t mode, int32_t *ind,
                  double *logq, double *val, bool dev)
{
    if (npts < 0 || (npts > 0 && (!u || !ind))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    int rc = sq_check_mode_gamma(who, mode, gamma);
    if (rc || (rc = check_train_one_process(h, who)) || (rc = sm_check_fixed(h, who, fixed))) return rc;
    const int d = h->d;
    std::vector<int> fx(d, 0);
    if (fixed) fx.assign(fixed, fixed + d);
    SmStage out[3] = {{ind, sizeof(int) * (size_t)d, SC_IND, nullptr}, {logq, sizeof(double), SC_LQ, nullptr}, {val, sizeof(double), SC_OUT, nullptr}};
    const auto state = [](const SqAt &a) { SqState st{a.state, nullptr}; st.fail = (int *)(st.lq + a.chunk); return st; };
    return sq_frame(h, who, SqKind{SMP_SQ, 1, 16, sizeof(double) + sizeof(int)}, npts, u, mode, dev, fx, out, 3,
        [&](const SqPlan &pl) {
            if (w) { const long long j = sq_bad_weight(w, pl.woff[d]); if (j >= 0) return fail(TTX_EINVAL, "%s: weight %lld is %g (finite and >= 0 expected: its square root enters)", who, j + 1, w[j]); }
            return (int)TTX_OK;
        },
        [&](const SqPlan &pl, SqHead &Qh) {
            std::vector<double> eff, gw;
            sq_effective(d, h->n1.data() + 1, fx.data(), w, gamma, eff, gw);
            return sq_head(h, pl, eff, fx, gw, Qh);
        },
        [&](auto ks, const SqAt &a, dim3 g, int tper) {
            hipLaunchKernelGGL(k_sq_rows_mfma<decltype(ks)::value>, g, dim3(256), 0, h->stream, a.Hk, a.l, a.n, a.r1, a.Xo, a.ldx, a.C, tper, a.S);
        },
        [&](const SqAt &a, dim3 g) { hipLaunchKernelGGL(k_sq_rows_exact, g, dim3(256), 0, h->stream, a.Hk, a.l, a.n, a.r1, a.Xo, a.ldx, a.C, a.S); },
        [&](const SqAt &a) {
            const SqState st = state(a);
            hipLaunchKernelGGL(k_sq_pick, dim3(a.grid), dim3(256), 0, h->stream, a.n, a.k, d, fx[a.k] - 1, a.Q->fixed, a.Q->w + a.woff, (const double *)(a.Q->g + a.k),
                               (const double *)a.S, st, (long long)a.C, a.du, a.first, a.last, (int *)out[0].dev, (double *)out[1].dev);
            hipLaunchKernelGGL(k_sq_step, dim3(a.grid), dim3(256), 0, h->stream, (const double *)core_dev(h, a.k + 1), h->RM, h->P.SS, a.r0, a.r1, a.n, a.k, d,
                               (const int *)out[0].dev, (const int *)st.fail, a.Xo, a.Xn, a.ldx, (long long)a.C, a.first, a.last, (double *)out[2].dev);
        },
        [&](size_t c, long long *dcnt) { hipLaunchKernelGGL(k_sm_count, dim3(1), dim3(1024), 0, h->stream, (long long)c, d, (const int *)out[0].dev, dcnt); });
}
extern "C" int ttx_sample_sq(ttx_engine *h, int64_t npts, const double *u, const double *w, const int32_t *fixed, double gamma, int32_t mode, int32_t *ind, double *logq,
                             double *val)
{
    return sq_run(h, "ttx_sample_sq", npts, u, w, fixed, gamma, mode, ind, logq, val, false);
}
extern "C" int ttx_sample_sq_dev(ttx_engine *h, int64_t npts, const double *u, const double *w, const int32_t *fixed, double gamma, int32_t mode, int32_t *ind, double *logq,
                                 double *val)
{
    return sq_run(h, "ttx_sample_sq_dev", npts, u, w, fixed, gamma, mode, ind, logq, val, true);
}
extern "C" int ttx_sample_sq_last(const ttx_engine *h, double *ms_head, double *ms_rows, double *ms_pick, double *flops, int64_t *nfailed, int32_t *mode_ran)
{
    return sq_last(h, "ttx_sample_sq_last", SMP_SQ, ms_head, ms_rows, ms_pick, flops, nfailed, mode_ran);
}

// ---- real-valued samples from the square of the interpolant of the resident train (ttx_sample_sq_real.h) -------------------------
// What ttx_sample_sq_real and its way back ttx_rosenblatt_sq_real share: everything but one launch.  in: the [npts][d] input (u, or x on the
// way back); rows: the [npts][d] output of doubles (x, or u on the way back), whose NaN rows k_sr_count counts; all five with cell, logq
// and val are host pointers (dev false: staged chunk by chunk) or pointers on the engine's device.  which: the caller's SampleLast slot.
// pick(a, M, st, out): the caller's launch between the rows and the step of a mode (k_sqr_pick, k_sqr_cdf), out[0 .. 2] = rows, cell, logq.
// Two sheets (squares and neighbour products), index tiles that advance by 15, per sample logq, the two hat values, the failure flag and
// the hat cell (SqrState)
// The head of ttx_sample_sq_real, of its way back and of a layer of TTX_FUN_PULLBACK (pb_prepare): the bidiagonal factors -- the mass
// matrix's Cholesky factor of a drawn mode, the hat row of a held one (a mode of one node is held at its node) --, the modes' records
// and sq_head with them
static int sqr_head(ttx_engine *h, const SqPlan &pl, const std::vector<int> &fx, const double *const *nodes, const double *cond, double gamma, std::vector<SrMode> &modes,
                    SqHead &Qh)
{
    const int d = h->d;
    std::vector<double> dg(pl.woff[d], 0.0), sp(pl.woff[d], 0.0), tnodes, gw(d + 1, gamma);
    for (int k = 0; k < d; k++) {
        const int n = h->n1[k + 1];
        const double *t = nodes[k];
        SrMode &M = modes[k];
        M = SrMode{0, 0, 1.0, 0.0, 0.0, tnodes.size()};
        tnodes.insert(tnodes.end(), t, t + n);
        double *dk = dg.data() + pl.woff[k], *sk = sp.data() + pl.woff[k];
        if (!fx[k]) { sqr_mass_cholesky(t, n, dk, sk); gw[k + 1] = gw[k] * (t[n - 1] - t[0]); continue; }
        M = sr_held_mode(t, n, cond && cond[k] == cond[k] ? cond[k] : t[0], M.noff);
        dk[M.cell] = M.phi0; sk[M.cell] = M.phi1;
        gw[k + 1] = gw[k];
    }
    return sq_head(h, pl, dg, fx, gw, Qh, &sp, &tnodes);
}
template <class Pick>
static int sqr_frame(ttx_engine *h, const char *who, int which, int64_t npts, const double *in, const double *const *nodes, const double *cond, double gamma, int32_t mode,
                     double *rows, int32_t *cell, double *logq, double *val, bool dev, Pick pick)
{
    if (npts < 0 || (npts > 0 && (!in || !rows || !nodes))) return fail(TTX_EINVAL, "%s: null argument or negative npts", who);
    int rc = sq_check_mode_gamma(who, mode, gamma);
    if (rc || (rc = check_train_one_process(h, who)) || (rc = sr_check_nodes_cond(h, who, nodes, cond))) return rc;
    const int d = h->d;
    std::vector<int> fx(d, 0);
    if (nodes) for (int k = 0; k < d; k++) fx[k] = (cond && cond[k] == cond[k]) || h->n1[k + 1] == 1;
    std::vector<SrMode> modes(d);
    SmStage out[4] = {{rows, sizeof(double) * (size_t)d, SC_SRX, nullptr}, {cell, sizeof(int) * (size_t)d, SC_IND, nullptr}, {logq, sizeof(double), SC_LQ, nullptr},
                      {val, sizeof(double), SC_OUT, nullptr}};
    const auto state = [](const SqAt &a) {
        SqrState st{a.state, nullptr, nullptr, nullptr, nullptr};
        st.f0 = st.lq + a.chunk; st.f1 = st.f0 + a.chunk;
        st.fail = (int *)(st.f1 + a.chunk); st.ci = st.fail + a.chunk;
        return st;
    };
    return sq_frame(h, who, SqKind{which, 2, 15, 3 * sizeof(double) + 2 * sizeof(int)}, npts, in, mode, dev, fx, out, 4,
        [](const SqPlan &) { return (int)TTX_OK; },
        [&](const SqPlan &pl, SqHead &Qh) { return sqr_head(h, pl, fx, nodes, cond, gamma, modes, Qh); },
        [&](auto ks, const SqAt &a, dim3 g, int tper) {
            hipLaunchKernelGGL(k_sqr_rows_mfma<decltype(ks)::value>, g, dim3(256), 0, h->stream, a.Hk, a.l, a.n, a.r1, a.Xo, a.ldx, a.C, tper, a.S, a.S + a.sheet);
        },
        [&](const SqAt &a, dim3 g) { hipLaunchKernelGGL(k_sqr_rows_exact, g, dim3(256), 0, h->stream, a.Hk, a.l, a.n, a.r1, a.Xo, a.ldx, a.C, a.S, a.S + a.sheet); },
        [&](const SqAt &a) {
            const SqrState st = state(a);
            pick(a, modes[a.k], st, out);
            hipLaunchKernelGGL(k_sqr_step, dim3(a.grid), dim3(256), 0, h->stream, (const double *)core_dev(h, a.k + 1), h->RM, h->P.SS, a.r0, a.r1, a.n, st, a.Xo, a.Xn, a.ldx,
                               (long long)a.C, a.last, (double *)out[3].dev);
        },
        [&](size_t c, long long *dcnt) { hipLaunchKernelGGL(k_sr_count, dim3(1), dim3(1024), 0, h->stream, (long long)c, d, (const double *)out[0].dev, dcnt); });
}
static int sqr_run(ttx_engine *h, const char *who, int64_t npts, const double *u, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *x,
                   int32_t *cell, double *logq, double *val, bool dev)
{
    return sqr_frame(h, who, SMP_SQ_REAL, npts, u, nodes, cond, gamma, mode, x, cell, logq, val, dev, [&](const SqAt &a, const SrMode &M, const SqrState &st, const SmStage *out) {
        hipLaunchKernelGGL(k_sqr_pick, dim3(a.grid), dim3(256), 0, h->stream, a.n, a.k, h->d, M, a.Q->fixed, a.Q->nodes, (const double *)(a.Q->g + a.k), (const double *)a.S,
                           (const double *)(a.S + a.sheet), st, (long long)a.C, a.du, a.first, a.last, (double *)out[0].dev, (int *)out[1].dev, (double *)out[2].dev);
    });
}
extern "C" int ttx_sample_sq_real(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *x,
                                  int32_t *cell, double *logq, double *val)
{
    return sqr_run(h, "ttx_sample_sq_real", npts, u, nodes, cond, gamma, mode, x, cell, logq, val, false);
}
extern "C" int ttx_sample_sq_real_dev(ttx_engine *h, int64_t npts, const double *u, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *x,
                                      int32_t *cell, double *logq, double *val)
{
    return sqr_run(h, "ttx_sample_sq_real_dev", npts, u, nodes, cond, gamma, mode, x, cell, logq, val, true);
}
extern "C" int ttx_sample_sq_real_last(const ttx_engine *h, double *ms_head, double *ms_rows, double *ms_pick, double *flops, int64_t *nfailed, int32_t *mode_ran)
{
    return sq_last(h, "ttx_sample_sq_real_last", SMP_SQ_REAL, ms_head, ms_rows, ms_pick, flops, nfailed, mode_ran);
}

// ---- the way back: the forward Rosenblatt map of the squared interpolant (k_sqr_cdf, ttx_sample_sq_real.h) -----------------------
// x goes where the sampler's u goes; u is the output whose NaN rows are counted
static int ros_run(ttx_engine *h, const char *who, int64_t npts, const double *x, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *u,
                   int32_t *cell, double *logq, double *val, bool dev)
{
    return sqr_frame(h, who, SMP_ROS_SQ_REAL, npts, x, nodes, cond, gamma, mode, u, cell, logq, val, dev, [&](const SqAt &a, const SrMode &M, const SqrState &st, const SmStage *out) {
        hipLaunchKernelGGL(k_sqr_cdf, dim3(a.grid), dim3(256), 0, h->stream, a.n, a.k, h->d, M, a.Q->nodes, (const double *)(a.Q->g + a.k), (const double *)a.S,
                           (const double *)(a.S + a.sheet), st, (long long)a.C, a.du, a.first, a.last, (double *)out[0].dev, (int *)out[1].dev, (double *)out[2].dev);
    });
}
extern "C" int ttx_rosenblatt_sq_real(ttx_engine *h, int64_t npts, const double *x, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *u,
                                      int32_t *cell, double *logq, double *val)
{
    return ros_run(h, "ttx_rosenblatt_sq_real", npts, x, nodes, cond, gamma, mode, u, cell, logq, val, false);
}
extern "C" int ttx_rosenblatt_sq_real_dev(ttx_engine *h, int64_t npts, const double *x, const double *const *nodes, const double *cond, double gamma, int32_t mode, double *u,
                                          int32_t *cell, double *logq, double *val)
{
    return ros_run(h, "ttx_rosenblatt_sq_real_dev", npts, x, nodes, cond, gamma, mode, u, cell, logq, val, true);
}
extern "C" int ttx_rosenblatt_sq_real_last(const ttx_engine *h, double *ms_head, double *ms_rows, double *ms_cdf, double *flops, int64_t *nfailed, int32_t *mode_ran)
{
    return sq_last(h, "ttx_rosenblatt_sq_real_last", SMP_ROS_SQ_REAL, ms_head, ms_rows, ms_cdf, flops, nfailed, mode_ran);
}

// ---- TTX_FUN_PULLBACK: layers, their heads and device blocks, the list entries (kernels in ttx_pullback.h, rules in ttx_pullback_plan.h) ----
// What the layers must be, for the set call and again before every evaluation (the caller may have changed a layer in between):
// pb_check on their shapes as they stand now, then the launch shape for the largest rank and mode over the layers against a
// workgroup's LDS.  x, nodes, gamma: the m layers (null lists: pb_check refuses them)
static int pb_check_layers(ttx_engine *h, const char *who, int m, ttx_engine *const *x, const double *const *const *nodes, const double *gamma, const double *const *ref,
                           PbPlan *plan, int *ldx_out, int *nmax_out)
{
    const int d = h->d, mm = (x && nodes && gamma && m >= 1 && m <= TTX_PULLBACK_MAX) ? m : 0;
    std::vector<PbLayer> L(std::max(mm, 1));
    std::vector<std::vector<int>> nn(mm), rr(mm);
    for (int t = 0; t < mm; t++) {
        const ttx_engine *y = x[t];
        L[t].x = y; L[t].nodes = nodes[t]; L[t].gamma = gamma[t];
        if (!y) continue;
        L[t].has_train = y->ran; L[t].one_process = y->W == 1; L[t].device = y->cfg.device; L[t].d = y->d;
        if (!y->ran) continue;
        nn[t].assign(y->n1.begin() + 1, y->n1.begin() + 1 + y->d); rr[t].assign(y->rfinal.begin(), y->rfinal.begin() + y->d + 1);
        L[t].n = nn[t].data(); L[t].r = rr[t].data();
    }
    std::string msg;
    if (int rc = pb_check(who, m, mm ? L.data() : nullptr, h, h->cfg.device, d, h->n1.data() + 1, ref, &msg)) return fail(rc, "%s", msg.c_str());
    int rmax = 1, nmax = 2;
    for (int t = 0; t < m; t++) { rmax = std::max(rmax, *std::max_element(rr[t].begin(), rr[t].end())); nmax = std::max(nmax, *std::max_element(nn[t].begin(), nn[t].end())); }
    const int ldx = (rmax + 3) & ~3;
    const PbPlan pl = pb_plan(ldx, nmax, d, dev_ncu(h), pb_env_grid(getenv("TTX_PB_GRID")));
    if (int rc = pb_check_lds(who, pl, ldx, nmax, d, &msg)) return fail(rc, "%s", msg.c_str());
    if (plan) *plan = pl;
    if (ldx_out) *ldx_out = ldx;
    if (nmax_out) *nmax_out = nmax;
    return TTX_OK;
}
extern "C" int ttx_set_integrand_pullback(ttx_engine *h, int32_t m, const ttx_layer *layer, const double *const *ref, const void *image, int64_t nbytes, const char *name,
                                          const double *par, int32_t npar)
{
    const char *who = "ttx_set_integrand_pullback";
    if (!h) return fail(TTX_EINVAL, "%s: null handle", who);
    if (h->cfg.fun_id != TTX_FUN_PULLBACK) return fail(TTX_ESTATE, "%s: the engine was not created with fun_id = TTX_FUN_PULLBACK", who);
    const int d = h->d, mm = (layer && m >= 1 && m <= TTX_PULLBACK_MAX) ? m : 0;
    std::vector<ttx_engine *> xs(mm);
    std::vector<const double *const *> nd(mm);
    std::vector<double> gm(mm);
    for (int t = 0; t < mm; t++) { xs[t] = layer[t].x; nd[t] = layer[t].nodes; gm[t] = layer[t].gamma; }
    HIPCHECK(hipSetDevice(h->cfg.device));
    if (int rc = pb_check_layers(h, who, m, layer ? xs.data() : nullptr, nd.data(), gm.data(), ref, nullptr, nullptr, nullptr)) return rc;   // before the code object is loaded
    std::shared_ptr<DevFun> c;
    if (image) {
        if (int rc = devfun_load(who, "ttx_devcomb_", "TTX_DEVICE_COMBINER", "combiner", h, image, nbytes, name, par, npar, &c)) return rc;
        if (c->info.kind != TTX_DEVFUN_KIND_LANE) return fail(TTX_EINVAL, "%s: combiner '%s' is not of the lane form", who, name);
    }
    auto f = std::make_shared<PullFun>();
    f->layer.resize(m);
    for (int t = 0; t < m; t++) {
        PullFun::Layer &Y = f->layer[t];
        Y.x = layer[t].x; Y.gamma = layer[t].gamma; Y.nodes.resize(d);
        for (int k = 0; k < d; k++) Y.nodes[k].assign(layer[t].nodes[k], layer[t].nodes[k] + Y.x->n1[k + 1]);
    }
    f->roff.resize(d);
    for (int k = 0; k < d; k++) { f->roff[k] = f->ref.size(); f->ref.insert(f->ref.end(), ref[k], ref[k] + h->n1[k + 1]); }
    f->comb = std::move(c);
    HIPCHECK(hipStreamSynchronize(h->stream));          // nothing of an earlier combiner is in flight when its module goes
    h->pfun = std::move(f);
    h->pb_ref_of = nullptr;
    return TTX_OK;
}
extern "C" int ttx_set_integrand_pullback_file(ttx_engine *h, int32_t m, const ttx_layer *layer, const double *const *ref, const char *path, const char *name,
                                               const double *par, int32_t npar)
{
    const char *who = "ttx_set_integrand_pullback_file";
    if (!h) return fail(TTX_EINVAL, "%s: null handle", who);
    if (h->cfg.fun_id != TTX_FUN_PULLBACK) return fail(TTX_ESTATE, "%s: the engine was not created with fun_id = TTX_FUN_PULLBACK", who);
    if (!path) return ttx_set_integrand_pullback(h, m, layer, ref, nullptr, 0, name, par, npar);
    std::vector<unsigned char> img;
    std::string text;
    if (int rc = devfun_read_file(who, path, img, &text)) return fail(rc, "%s", text.c_str());
    return ttx_set_integrand_pullback(h, m, layer, ref, img.data(), (int64_t)img.size(), name, par, npar);
}
// At the start of every call that evaluates: the layers checked again as they stand NOW; on each distinct layer engine sqr_frame's head
// (the mass matrices' Cholesky factors, gw and sq_head with sp and the nodes), on that engine's stream and in its own work space, and
// one wait per such engine; then the layers' blocks -- the plan's rows and offsets, core pointers, ranks, mode sizes -- into this
// engine's scratch (SC_PB), the reference rows once per set (SC_PBREF), the two counters (SC_CNT) and with a combiner the rows x, logq,
// val (SC_PBVAL).  figures: the call records what ttx_pullback_last reports (ttx_accchk leaves the last run's figures as they are).
static int pb_prepare(ttx_engine *h, const char *who, bool figures, bool need_comb)
{
    if (!h->pfun) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_pullback first", who);
    const PullFun &f = *h->pfun;
    if (need_comb && !f.comb) return fail(TTX_ESTATE, "%s: call ttx_set_integrand_pullback with a combiner first (the layers alone serve ttx_pullback_points)", who);
    const int m = (int)f.layer.size(), d = h->d;
    int rc, ldx = 4, nmax = 2;
    PbPlan plan;
    std::vector<ttx_engine *> xs(m);
    std::vector<std::vector<const double *>> rows(m, std::vector<const double *>(d));
    std::vector<const double *const *> nd(m);
    std::vector<double> gm(m);
    std::vector<const double *> refp(d);
    for (int t = 0; t < m; t++) {
        xs[t] = f.layer[t].x; gm[t] = f.layer[t].gamma;
        for (int k = 0; k < d; k++) rows[t][k] = f.layer[t].nodes[k].data();
        nd[t] = rows[t].data();
    }
    for (int k = 0; k < d; k++) refp[k] = f.ref.data() + f.roff[k];
    HIPCHECK(hipSetDevice(h->cfg.device));
    if ((rc = pb_check_layers(h, who, m, xs.data(), nd.data(), gm.data(), refp.data(), &plan, &ldx, &nmax))) return rc;
    // the heads: one per distinct layer engine
    std::vector<SqPlan> pls(m);
    std::vector<SqHead> Qs(m);
    std::vector<int> head_of(m);
    const std::vector<int> fx(d, 0);
    for (int t = 0; t < m; t++) {
        head_of[t] = t;
        for (int s = 0; s < t; s++) if (xs[s] == xs[t]) { head_of[t] = s; break; }
        if (head_of[t] != t) continue;
        ttx_engine *y = xs[t];
        std::vector<SrMode> modes(d);
        sq_plan(d, y->n1.data() + 1, y->rfinal.data(), fx.data(), pls[t]);
        if ((rc = tt_prepare(y, who)) || (rc = sqr_head(y, pls[t], fx, nd[t], nullptr, gm[t], modes, Qs[t]))) return rc;
    }
    for (int t = 0; t < m; t++) if (head_of[t] == t) HIPCHECK(hipStreamSynchronize(xs[t]->stream));
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipSetDevice(h->cfg.device));
    OpMeta meta(h->pb_host);
    size_t o_l[TTX_PULLBACK_MAX], o_hoff[TTX_PULLBACK_MAX], o_woff[TTX_PULLBACK_MAX], o_core[TTX_PULLBACK_MAX], o_r[TTX_PULLBACK_MAX], o_n[TTX_PULLBACK_MAX];
    for (int t = 0; t < m; t++) {
        const ttx_engine *y = xs[t];
        const SqPlan &pl = pls[head_of[t]];
        std::vector<const double *> cp(d);
        for (int k = 1; k <= d; k++) cp[k - 1] = core_dev(y, k);
        o_l[t] = meta.put(pl.l); o_hoff[t] = meta.put(pl.hoff); o_woff[t] = meta.put(pl.woff); o_core[t] = meta.put(cp);
        o_r[t] = meta.put(std::vector<int>(y->rfinal.begin(), y->rfinal.begin() + d + 1));
        o_n[t] = meta.put(std::vector<int>(y->n1.begin() + 1, y->n1.begin() + 1 + d));
    }
    const size_t o_en = meta.put(std::vector<int>(h->n1.begin() + 1, h->n1.begin() + 1 + d));
    char *dm;
    if ((rc = meta.upload(h, SC_PB, &dm)) || (rc = buf_reserve(h, SC_CNT, 2 * sizeof(long long)))) return rc;
    const size_t refbytes = sizeof(double) * f.ref.size(), roffat = (refbytes + 15) & ~(size_t)15;
    if ((rc = buf_reserve(h, SC_PBREF, roffat + sizeof(size_t) * d))) return rc;
    if (h->pb_ref_of != &f) {
        HIPCHECK(hipMemcpyAsync(buf<char>(h, SC_PBREF), f.ref.data(), refbytes, hipMemcpyHostToDevice, h->stream));
        HIPCHECK(hipMemcpyAsync(buf<char>(h, SC_PBREF) + roffat, f.roff.data(), sizeof(size_t) * d, hipMemcpyHostToDevice, h->stream));
        h->pb_ref_of = &f;
    }
    if (f.comb && (rc = buf_reserve(h, SC_PBVAL, sizeof(double) * (size_t)h->G * h->sel.HS * (d + 2)))) return rc;
    HIPCHECK(hipMemsetAsync(buf<char>(h, SC_CNT), 0, 2 * sizeof(long long), h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    if ((rc = op_lds_raise(h, reinterpret_cast<const void *>(k_pb_slots), op_lds(plan.lds))) || (rc = op_lds_raise(h, reinterpret_cast<const void *>(k_pb_list), op_lds(plan.lds))))
        return rc;
    PbOps &O = h->pb_ops;
    O = PbOps{};
    O.m = m; O.d = d; O.ldx = ldx; O.nmax = nmax; O.n = (const int *)(dm + o_en);
    O.ref = (const double *)buf<char>(h, SC_PBREF); O.roff = (const size_t *)(buf<char>(h, SC_PBREF) + roffat);
    for (int t = 0; t < m; t++) {
        const SqHead &Q = Qs[head_of[t]];
        PbLayerDev &Y = O.t[t];
        Y.H = Q.H; Y.g = Q.g; Y.nodes = Q.nodes;
        Y.l = (const int *)(dm + o_l[t]); Y.hoff = (const size_t *)(dm + o_hoff[t]); Y.woff = (const size_t *)(dm + o_woff[t]);
        Y.core = (const double *const *)(dm + o_core[t]); Y.r = (const int *)(dm + o_r[t]); Y.n = (const int *)(dm + o_n[t]);
        Y.RM = xs[t]->RM; Y.SS = xs[t]->P.SS;
    }
    h->pb_pl = plan;
    h->tf_figures = figures;
    if (!figures) return TTX_OK;
    h->tf_launches = 0; h->tf_elements = 0; h->tf_ms = 0.0; h->pb_failed = 0;
    for (auto &e : h->tf_evs) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    h->tf_evs.clear();
    return TTX_OK;
}
// k_pb_slots over all slots of this process behind pass 1, and the loaded combiner's slot kernel behind that over tval [nslot][d+2]: no
// synchronisation
static int pb_slots(ttx_engine *h)
{
    DevFun &c = *h->pfun->comb;
    DevProb &P = h->P;
    long long nslot = (long long)h->G * h->sel.HS;
    const PbOps &O = h->pb_ops;
    const PbPlan &pl = h->pb_pl;
    const short *hidx = P.hidx; unsigned char *hreq = P.hreq; double *hval = P.hval;
    double *tval = buf<double>(h, SC_PBVAL);
    unsigned long long *cnt = buf<unsigned long long>(h, SC_CNT);
    if (h->tf_figures) h->tf_launches++;
    TfScope timed(h);
    hipLaunchKernelGGL(k_pb_slots, dim3(pl.grid(nslot)), dim3(64 * pl.waves), pl.lds, h->stream, O, nslot, hidx, (const unsigned char *)hreq, tval, cnt);
    int m = O.d + 2, d = O.d;
    const int *n = P.n + 1;
    const double *par = c.par, *tv = tval;
    const unsigned cg = (unsigned)std::max<long long>(1, std::min<long long>((nslot + c.info.block - 1) / c.info.block, 4096));
    void *args[] = {&m, &d, &n, &par, &nslot, &hidx, &hreq, &tv, &hval};
    DEVFUN_LAUNCHCHECK(hipModuleLaunchKernel(c.slots, cg, 1, 1, (unsigned)c.info.block, 1, 1, 0, h->stream, args, nullptr));
    return TTX_OK;
}
// after the last launch of a call: the elements the transport kernel evaluated, the failed ones and, with ttx_set_profile on, its milliseconds
static int pb_finish(ttx_engine *h)
{
    unsigned long long c[2] = {0, 0};
    HIPCHECK(hipMemcpyAsync(c, buf<char>(h, SC_CNT), sizeof c, hipMemcpyDeviceToHost, h->stream));
    HIPCHECK(hipStreamSynchronize(h->stream));
    h->tf_elements = (int64_t)c[0]; h->pb_failed = (int64_t)c[1];
    for (auto &e : h->tf_evs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess) h->tf_ms += ms;
        (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    h->tf_evs.clear();
    return TTX_OK;
}
// the two list entries: k_pb_list over the staged rows, in chunks; out != null: the combiner's list kernel behind it (ttx_eval_device),
// otherwise x, logq, val themselves (ttx_pullback_points; logq, val may be null)
static int pb_list(ttx_engine *h, const char *who, int64_t npts, const int32_t *ind, double *out, double *x, double *logq, double *val)
{
    const bool comb = out != nullptr;
    if (npts < 0 || (npts > 0 && (!ind || !(out || x)))) return fail(TTX_EINVAL, "%s: null argument", who);
    int rc = pb_prepare(h, who, true, comb);
    if (rc) return rc;
    if (npts == 0) return TTX_OK;
    const int d = h->d;
    for (int64_t p = 0; p < npts; p++)
        for (int k = 0; k < d; k++)
            if (ind[p * d + k] < 1 || ind[p * d + k] > h->n1[k + 1])
                return fail(TTX_EINVAL, "%s: point %lld: index %d of mode %d is outside 1..%d", who, (long long)p, ind[p * d + k], k + 1, h->n1[k + 1]);
    const PbOps &O = h->pb_ops;
    const PbPlan &pl = h->pb_pl;
    const size_t chunk = (size_t)std::min<int64_t>(npts, 1 << 16);
    if ((rc = buf_reserve(h, SC_IND, sizeof(int) * chunk * d)) || (rc = buf_reserve(h, SC_OUT, sizeof(double) * chunk))) return rc;
    if (comb) { if ((rc = buf_reserve(h, SC_PBVAL, sizeof(double) * std::max(chunk, (size_t)h->G * h->sel.HS) * (d + 2)))) return rc; }
    else if ((rc = buf_reserve(h, SC_SRX, sizeof(double) * chunk * d)) || (rc = buf_reserve(h, SC_LQ, sizeof(double) * chunk))) return rc;
    int *sind = buf<int>(h, SC_IND);
    double *sout = buf<double>(h, SC_OUT), *sx = comb ? nullptr : buf<double>(h, SC_SRX), *slq = comb ? nullptr : buf<double>(h, SC_LQ), *tval = comb ? buf<double>(h, SC_PBVAL) : nullptr;
    unsigned long long *cnt = buf<unsigned long long>(h, SC_CNT);
    for (int64_t o = 0; o < npts; o += (int64_t)chunk) {
        long long c = std::min<int64_t>((int64_t)chunk, npts - o);
        HIPCHECK(hipMemcpyAsync(sind, ind + (size_t)o * d, sizeof(int) * (size_t)c * d, hipMemcpyHostToDevice, h->stream));
        h->tf_launches++;
        {
            TfScope timed(h);
            hipLaunchKernelGGL(k_pb_list, dim3(pl.grid(c)), dim3(64 * pl.waves), pl.lds, h->stream, O, c, (const int *)sind, sx, slq, sout, tval, cnt);
            if (comb) {
                DevFun &cb = *h->pfun->comb;
                int m = d + 2, dd = d;
                const int *n = h->P.n + 1, *ip = sind;
                const double *par = cb.par, *tv = tval;
                const unsigned cg = (unsigned)std::max<long long>(1, std::min<long long>((c + cb.info.block - 1) / cb.info.block, 4096));
                void *args[] = {&m, &dd, &n, &par, &c, &ip, &tv, &sout};
                DEVFUN_LAUNCHCHECK(hipModuleLaunchKernel(cb.list, cg, 1, 1, (unsigned)cb.info.block, 1, 1, 0, h->stream, args, nullptr));
            }
        }
        if (comb) HIPCHECK(hipMemcpyAsync(out + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
        else {
            HIPCHECK(hipMemcpyAsync(x + (size_t)o * d, sx, sizeof(double) * (size_t)c * d, hipMemcpyDeviceToHost, h->stream));
            if (logq) HIPCHECK(hipMemcpyAsync(logq + o, slq, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
            if (val) HIPCHECK(hipMemcpyAsync(val + o, sout, sizeof(double) * (size_t)c, hipMemcpyDeviceToHost, h->stream));
        }
        HIPCHECK(hipStreamSynchronize(h->stream));
    }
    HIPCHECK(hipGetLastError());
    return pb_finish(h);
}
static int pb_eval_list(ttx_engine *h, int64_t npts, const int32_t *ind, double *out)
{
    if (npts > 0 && !out) return fail(TTX_EINVAL, "ttx_eval_device: null argument");
    double none = 0.0;
    return pb_list(h, "ttx_eval_device", npts, ind, out ? out : &none, nullptr, nullptr, nullptr);
}
extern "C" int ttx_pullback_points(ttx_engine *h, int64_t npts, const int32_t *ind, double *x, double *logq, double *val)
{
    const char *who = "ttx_pullback_points";
    if (!h) return fail(TTX_EINVAL, "%s: null handle", who);
    if (h->cfg.fun_id != TTX_FUN_PULLBACK) return fail(TTX_ESTATE, "%s: the engine was not created with fun_id = TTX_FUN_PULLBACK", who);
    if (npts > 0 && !x) return fail(TTX_EINVAL, "%s: null argument", who);
    double none = 0.0;
    return pb_list(h, who, npts, ind, nullptr, x ? x : &none, logq, val);
}
extern "C" int ttx_pullback_last(const ttx_engine *h, double *ms, int64_t *launches, int64_t *elements, int64_t *nfailed)
{
    if (!h) return fail(TTX_EINVAL, "ttx_pullback_last: null handle");
    if (ms) *ms = h->tf_ms;
    if (launches) *launches = h->tf_launches;
    if (elements) *elements = h->tf_elements;
    if (nfailed) *nfailed = h->pb_failed;
    return TTX_OK;
}

extern "C" int ttx_kernel_stats(const ttx_engine *h, int64_t launches[TTX_K_NKINDS], double ms[TTX_K_NKINDS], double bytes[TTX_K_NKINDS])
{
    if (!h) return fail(TTX_EINVAL, "null");
    for (int k = 0; k < TTX_K_NKINDS; k++) { launches[k] = h->k_launches[k]; ms[k] = h->k_ms[k]; bytes[k] = h->k_bytes[k]; }
    return TTX_OK;
}

extern "C" int ttx_exp_host(int64_t n, const double *x, double *out)
{
    if (!x || !out || n < 0) return fail(TTX_EINVAL, "ttx_exp_host: bad argument");
    for (int64_t i = 0; i < n; i++) out[i] = ttx_exp(x[i]);
    return TTX_OK;
}

// the fast evaluators' tables of one bond as a run left them (read-only): side 0 = left pivots of bond `bond` (first-1 .. last of
// the group), side 1 = right pivots of bond `bond` (first .. last+1).  info = {live pivots r of the bond, first, last}; with idx = null
// only info[1..2] are set (any bond).  Compact copies, r columns each: idx [d][r], near / dv [d+1][r], piv [8][r]; cols = columns the
// caller's buffers hold
extern "C" int ttx_fast_tables(const ttx_engine *h, int32_t group, int32_t side, int32_t bond, int32_t cols, int32_t *info, int32_t *idx, double *near,
                               double *dv, double *piv)
{
    if (!h || !info) return fail(TTX_EINVAL, "ttx_fast_tables: null argument");
    if (!h->ran) return fail(TTX_ESTATE, "ttx_fast_tables: run first");
    const DevProb &P = h->P;
    if (!P.arith || !P.fNear[0] || !P.fpersist) return fail(TTX_ESTATE, "ttx_fast_tables: this engine keeps no per-bond tables (TTX_ARITH=fast with Ising D/E or mvn)");
    if (group < 0 || group >= h->G || side < 0 || side > 1) return fail(TTX_EINVAL, "ttx_fast_tables: group %d / side %d out of range", group, side);
    const int first = h->own[h->g0 + group], last = h->own[h->g0 + group + 1] - 1;
    info[0] = 0; info[1] = first; info[2] = last;
    if (!idx) return TTX_OK;
    if (!near || !piv || (P.fDv[side] && !dv)) return fail(TTX_EINVAL, "ttx_fast_tables: null argument");
    const int lo = side == 0 ? first - 1 : first, hi = side == 0 ? last : last + 1;
    if (bond < lo || bond > hi) return fail(TTX_EINVAL, "ttx_fast_tables: bond %d outside %d..%d of group %d, side %d", bond, lo, hi, group, side);
    const int d = h->d;
    const size_t RM = h->RM, slot = (size_t)group * h->NC + (size_t)(side == 0 ? bond - first + 1 : bond - first);     // fast_slot, L_ptr / R_ptr
    std::vector<int> rr(d + 2);
    HIPCHECK(hipMemcpy(rr.data(), P.r + (size_t)group * (d + 2), sizeof(int) * (d + 2), hipMemcpyDeviceToHost));
    const int r = rr[bond];
    if (r < 1 || (size_t)r > RM || r > cols) return fail(TTX_EINVAL, "ttx_fast_tables: bond %d has %d pivots, the buffers hold %d", bond, r, cols);
    info[0] = r;
    std::vector<short> tab((size_t)d * RM);
    HIPCHECK(hipMemcpy(tab.data(), (side == 0 ? P.L : P.R) + slot * (size_t)d * RM, sizeof(short) * tab.size(), hipMemcpyDeviceToHost));
    for (int x = 0; x < d; x++) for (int c = 0; c < r; c++) idx[(size_t)x * r + c] = tab[(size_t)x * RM + c];
    const size_t w = sizeof(double) * r, pitch = sizeof(double) * RM;
    HIPCHECK(hipMemcpy2D(near, w, P.fNear[side] + slot * (size_t)P.FD * RM, pitch, w, P.FD, hipMemcpyDeviceToHost));
    HIPCHECK(hipMemcpy2D(piv, w, P.fPiv[side] + slot * (size_t)TTX_FS * RM, pitch, w, TTX_FS, hipMemcpyDeviceToHost));
    if (P.fDv[side]) HIPCHECK(hipMemcpy2D(dv, w, P.fDv[side] + slot * (size_t)P.FD * RM, pitch, w, P.FD, hipMemcpyDeviceToHost));
    return TTX_OK;
}

#include "ttx_ktest.h"   // the test and probe entry points (ttx_k_*)
