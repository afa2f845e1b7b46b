// ttx_qr_plan.h -- which kernels factor an m x n unfolding, decided before anything is launched (host only, no HIP in here).
//
// qr_plan() is a pure function of the shape, of whether the matrix lies in the engine's first work buffer (the tall-skinny
// route keeps its panels in the other three) and of five environment switches; qr() in ttx_engine.hip raises the LDS ceilings
// of the plan's kernels and issues its launches in order.  tests/qr_plan_main.cpp prints and checks plans on the CPU.
#pragma once
#include <algorithm>
#include <cstddef>
#include <vector>

// dynamic-LDS budgets, in bytes: of the tt_lib utilities, and of the sweep's kernels as engine creation sizes them (ttx_create_plan.h)
constexpr size_t TTX_LDS_DEVICE = 160 * 1024;       // what a workgroup of the device can have; the half-step's staging may take all of it
constexpr size_t TTX_LDS_WORK = 150 * 1024;         // what a kernel's working set asks for at most: the one-workgroup QR kernels, the sweep's variants
constexpr size_t TTX_LDS_JACOBI = 140 * 1024;       // up to here the Jacobi SVD keeps X and V in LDS
constexpr size_t TTX_LDS_HALF_DIFF = 140 * 1024;    // up to here the mvn half-step keeps rows of differences x - mu instead of index rows
constexpr size_t TTX_LDS_LOTTERY = 120 * 1024;      // what the lottery kernel may stage; a problem that needs more is refused
constexpr size_t TTX_LDS_VALUES = 100 * 1024;       // up to here the Ising C half-step keeps value rows, and the fast lottery its decay-table rows
constexpr size_t TTX_LDS_FIN = 96 * 1024;           // the finalisation halves its workgroup until the LU panel and its columns are below this

// the switches, read per call by the engine (threads already clamped to a multiple of 64 in 64..1024)
struct QrEnv {
    bool own_off = false;           // TTX_QR_OWN=0: no register kernel
    bool tsqr_off = false;          // TTX_TSQR=0: no tall-skinny route
    int threads = 1024;             // TTX_QR_THREADS
    int top_threads = 1024;         // TTX_QRTOP_THREADS: k_qr<true> on top of LDS panels
    int panel = 0;                  // TTX_QR_PANEL: rows of a register panel (0: unset)
};

enum QrRoute { QR_REFUSED, QR_TSQR_REG, QR_TSQR_LDS, QR_ONE_REG, QR_LDS, QR_STREAM };
enum QrKernel { QRK_NONE, QRK_OWN, QRK_PANEL, QRK_LDS, QRK_STREAM };    // k_qr_own<MR, NC>, k_qr_panel, k_qr<true>, k_qr<false>

struct QrLaunch {
    QrKernel kernel = QRK_NONE;
    int rows = 0, P = 1, rbs = 0;   // P panels of rbs rows (P = 1, rbs = rows: the whole matrix)
    int mr = 0, nc = 0;             // k_qr_own's instantiation: rows per lane, columns per wave
    int threads = 0;
    size_t lds = 0;                 // bytes
};
// a level of the tall-skinny route; offsets in doubles: level 0 factors A itself into Q panels at Wb, a level l >= 1 factors
// the stacked triangles at Wc + m_off into Q panels at Wd + q_off; its own triangles (P n x n) go to Wc + r_off
struct QrLevel : QrLaunch { size_t m_off = 0, q_off = 0, r_off = 0; };
struct QrPlan {
    QrRoute route = QR_REFUSED;
    std::vector<QrLevel> lv;
    QrLaunch top;                   // one workgroup; after levels: in place at Wc + top_off
    size_t top_off = 0;
};

// the kernels' LDS formulas (ttx_ttops.h: qr_own_lds_doubles, qr_panel_lds_doubles; qr() checks that they agree)
inline size_t qr_plan_own_doubles(int m, int n) { return (size_t)((n + 2) & ~1) + (size_t)m * (m < n ? m : n); }
inline size_t qr_plan_panel_doubles(int rbs, int n) { return (size_t)((rbs + 2 * n + 1) & ~1) + (size_t)rbs * n; }

// k_qr_own<MR, NC> (matrix in registers, one barrier per reflector): NC = columns per wave, MR = rows per lane at most
struct QrOwnShape { int nt = 0, mr = 0, nc = 0, rows_cap = 0; };
inline QrOwnShape qr_own_shape(int n, const QrEnv &env)
{
    QrOwnShape s;
    if (n < 1 || n > 128 || env.own_off) return s;
    const int nw = env.threads / 64;
    int nc = 1; while (nc * nw < n) nc *= 2;
    if (nc > 8) return s;
    s.nt = env.threads;
    s.nc = nc;
    s.mr = nc <= 2 ? 8 : 4;                                                  // rows per lane the instantiations hold without spilling
    const size_t budget = TTX_LDS_WORK / sizeof(double);
    const long lds_rows = (long)((budget - (size_t)n - 4) / (size_t)n);
    s.rows_cap = (int)std::min<long>(64L * s.mr, lds_rows);
    return s;
}
// one launch of the register kernel over P panels of rbs rows; kernel stays QRK_NONE where no instantiation holds rbs rows
inline QrLaunch qr_own_launch(const QrOwnShape &s, int rows, int n, int rbs, int P)
{
    QrLaunch L;
    int mr = 1; while (mr * 64 < rbs) mr *= 2;
    if (mr < 2) mr = 2;
    if (!s.nt || mr > s.mr) return L;
    L.kernel = QRK_OWN; L.rows = rows; L.P = P; L.rbs = rbs; L.mr = mr; L.nc = s.nc; L.threads = s.nt;
    L.lds = sizeof(double) * qr_plan_own_doubles(rbs, n);
    return L;
}

// Tall-skinny QR of A (m x n, m >> n) over several workgroups: levels of panel factorisations side by side, then the explicit Q
// from the top level down.  false: shape not eligible (the plan is left untouched).
inline bool qr_plan_tsqr(QrPlan &out, int m, int n, bool a_is_Wa, const QrEnv &env)
{
    if (!a_is_Wa || n > 96 || m < 4 * n || env.tsqr_off) return false;
    const QrOwnShape own = qr_own_shape(n, env);
    const bool use_own = own.nt && own.rows_cap >= 2 * n;
    const size_t budget = TTX_LDS_WORK / sizeof(double);
    // rows of a panel: the register kernel's time per reflector grows with the rows per lane, so its panels are short (4 n rows,
    // at least 256 -- measured optimum for n = 32); the LDS kernel takes what fits with its reflector
    int RB = use_own ? std::min(own.rows_cap, std::max(256, 4 * n)) : (int)((budget - 2 * n - 2) / (size_t)(n + 1));
    if (use_own && env.panel >= 2 * n) RB = std::min(own.rows_cap, env.panel);
    if (RB < 2 * n) return false;
    QrPlan p;
    p.route = use_own ? QR_TSQR_REG : QR_TSQR_LDS;
    auto top_fits = [&](int rws) { return use_own ? rws <= own.rows_cap : (size_t)rws * n + rws + 2 * n + 4 <= budget; };
    int rows = m;
    size_t s_off = 0, t_off = 0, m_off = 0;                                     // next free double of Wc, of Wd; this level's matrix
    while (!top_fits(rows)) {                                                   // until one workgroup takes the rest
        const int P = (rows + RB - 1) / RB, rbs = (rows + P - 1) / P;
        if (rows - (P - 1) * rbs < n) return false;                             // a last panel shorter than n: keep the one-workgroup path
        QrLevel L;
        if (use_own) static_cast<QrLaunch &>(L) = qr_own_launch(own, rows, n, rbs, P);
        if (L.kernel == QRK_NONE) {
            L.kernel = QRK_PANEL; L.rows = rows; L.P = P; L.rbs = rbs; L.threads = env.threads;
            L.lds = sizeof(double) * qr_plan_panel_doubles(rbs, n);
        }
        L.m_off = m_off; L.r_off = s_off;
        if (!p.lv.empty()) { L.q_off = t_off; t_off += (size_t)rows * n; }
        p.lv.push_back(L);
        m_off = s_off; s_off += (size_t)P * n * n; rows = P * n;
    }
    // Wb, Wc and Wd hold at least the m n doubles of A: levels whose triangles need more of Wc keep the one-workgroup path (Wd takes
    // less than Wc).  Panels of little more than 2 n rows get there: 1632 x 96 would need 1.12 m n.
    if (p.lv.empty() || s_off > (size_t)m * n) return false;
    // top: one workgroup, in place
    if (use_own) p.top = qr_own_launch(own, rows, n, rows, 1);
    if (p.top.kernel == QRK_NONE) {
        p.top.kernel = QRK_LDS; p.top.rows = rows; p.top.rbs = rows; p.top.threads = env.top_threads;
        p.top.lds = sizeof(double) * ((size_t)rows + 2 * n + 4 + (size_t)rows * n);
    }
    p.top_off = m_off;
    out = p;
    return true;
}

inline QrPlan qr_plan(int m, int n, bool a_is_Wa, const QrEnv &env)
{
    QrPlan p;
    if (qr_plan_tsqr(p, m, n, a_is_Wa, env)) return p;
    p.top.rows = p.top.rbs = m;
    const QrOwnShape own = qr_own_shape(n, env);                               // small unfoldings: one workgroup, matrix in registers
    if (own.nt && m <= own.rows_cap) {
        const QrLaunch L = qr_own_launch(own, m, n, m, 1);
        if (L.kernel != QRK_NONE) { p.route = QR_ONE_REG; p.top = L; return p; }
    }
    const size_t lds = sizeof(double) * ((size_t)m + n + 4);
    if (lds > TTX_LDS_WORK) return p;                                           // refused: the reflector alone does not fit
    // small unfoldings are factored entirely inside LDS; larger ones stream the panel from L2 with threads mapped to rows
    const size_t lds_all = lds + sizeof(double) * ((size_t)m * n + n);
    if (lds_all <= TTX_LDS_WORK) { p.route = QR_LDS; p.top.kernel = QRK_LDS; p.top.threads = env.threads; p.top.lds = lds_all; }
    else { p.route = QR_STREAM; p.top.kernel = QRK_STREAM; p.top.threads = 1024; p.top.lds = lds; }
    return p;
}

inline const char *qr_route_name(QrRoute r)
{
    static const char *const names[] = {"refused", "tsqr_reg", "tsqr_lds", "one_reg", "qr_lds", "qr_stream"};
    return names[r];
}
