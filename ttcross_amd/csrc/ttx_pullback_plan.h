// ttx_pullback_plan.h -- TTX_FUN_PULLBACK: what a set call refuses and what a launch of k_pb_slots / k_pb_list takes, decided on the
// host before anything is launched (host only: no HIP in here beyond the qualifiers of the one formula the kernels share).
//
// The definition of the integrand is in include/ttx.h, the kernels are in ttx_pullback.h.  Everything here is a pure function of
// plain data -- the layers' shapes (PbLayer, filled by the engine from its handles), the node and reference rows, the device's CU
// count and TTX_PB_GRID -- so tests/pullback_plan_main.cpp runs it on the CPU.
//
// An engine that is two layers: both layers read ONE head (the tables H, g of sqr_frame's head pass, which live in the layer
// engine's own work space), so they must name the same nodes, value for value, and the same gamma.  Two layers of one engine with
// different nodes or gamma are REFUSED (pb_check); a private copy of H and g per layer in the pullback engine's scratch is open.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <string>

#include "../../include/ttx.h"      // TTX_OK, TTX_EINVAL, TTX_PULLBACK_MAX
#include "ttx_qr_plan.h"            // TTX_LDS_WORK

#if defined(__HIPCC__)
#define TTX_PB_HD __host__ __device__ inline
#else
#define TTX_PB_HD inline
#endif

#define TTX_PB_WAVES 4              // waves per workgroup at most
#define TTX_PB_RMAX 128             // the samplers' rank cap

// doubles of dynamic LDS per wave: two state vectors x[ldx], z[ldx], the two sheets s[nmax], c[nmax] of the largest mode over the
// layers, the running point u[d] (x_k overwrites u_k), the index row id[d] as ints
TTX_PB_HD size_t pb_lds_doubles(int ldx, int nmax, int d) { return 2 * (size_t)ldx + 2 * (size_t)nmax + (size_t)d + (((size_t)d + 1) >> 1); }

// the launch shape: one wave64 per item, `waves` per workgroup (at most TTX_PB_WAVES, halved until the workgroup's LDS is within
// TTX_LDS_WORK), a capped grid that strides.  refused: one wave alone needs more than TTX_LDS_WORK
struct PbPlan {
    size_t per_wave = 0;            // doubles
    int waves = 0;
    size_t lds = 0;                 // bytes of the workgroup
    bool raise = false;             // above the default ceiling of 64 KB: the kernel's attribute is raised first
    bool refused = false;
    int grid_cap = 1;               // workgroups: 8 per CU, less where TTX_PB_GRID names fewer
    int grid(long long items) const { return (int)std::max<long long>(1, std::min<long long>((items + waves - 1) / std::max(waves, 1), grid_cap)); }
};
// env_grid: TTX_PB_GRID as a number, < 1: not set
inline PbPlan pb_plan(int ldx, int nmax, int d, int ncu, long long env_grid)
{
    PbPlan p;
    p.per_wave = pb_lds_doubles(ldx, nmax, d);
    p.waves = TTX_PB_WAVES;
    while (p.waves > 1 && sizeof(double) * p.per_wave * p.waves > TTX_LDS_WORK) p.waves >>= 1;
    p.lds = sizeof(double) * p.per_wave * p.waves;
    p.refused = p.lds > TTX_LDS_WORK;
    p.raise = p.lds > 64 * 1024;
    long long cap = (long long)std::max(ncu, 1) * 8;
    if (env_grid >= 1) cap = std::min(cap, env_grid);
    p.grid_cap = (int)cap;
    return p;
}
inline long long pb_env_grid(const char *e) { return e && *e ? atoll(e) : 0; }

// ---- the refusals of a set call -----------------------------------------------------------------------------------------------------
// a node row of a layer: n >= 2 finite, strictly ascending nodes; unit: the ends are exactly 0.0 and 1.0 (layers 2 and up, whose
// output feeds the next layer as uniforms).  Empty string: the row is accepted
inline std::string pb_bad_nodes(const double *t, int n, bool unit)
{
    char b[160];
    if (!t) return "is missing";
    for (int i = 0; i < n; i++) if (!(fabs(t[i]) <= 1.7976931348623157e308)) { snprintf(b, sizeof b, "node %d is %g (finite expected)", i + 1, t[i]); return b; }
    for (int i = 0; i + 1 < n; i++) if (!(t[i] < t[i + 1])) { snprintf(b, sizeof b, "nodes %d and %d are %g and %g (strictly ascending expected)", i + 1, i + 2, t[i], t[i + 1]); return b; }
    if (unit && !(t[0] == 0.0 && t[n - 1] == 1.0)) {
        snprintf(b, sizeof b, "ends at %.17g and %.17g (exactly 0 and 1 expected: the layer's output is the next layer's uniforms)", t[0], t[n - 1]);
        return b;
    }
    return "";
}
// a row of the reference grid: n entries in [0, 1] (a NaN is outside)
inline std::string pb_bad_ref(const double *u, int n)
{
    char b[160];
    if (!u) return "is missing";
    for (int i = 0; i < n; i++) if (!(u[i] >= 0.0 && u[i] <= 1.0)) { snprintf(b, sizeof b, "entry %d is %g (0 <= u <= 1 expected)", i + 1, u[i]); return b; }
    return "";
}

// one layer as the checks see it; the engine fills it from the layer's handle
struct PbLayer {
    const void *x = nullptr;        // the handle (identity only)
    bool has_train = false, one_process = true;
    int device = 0, d = 0;
    const int *n = nullptr;         // [d] mode sizes (null without a train)
    const int *r = nullptr;         // [d+1] ranks
    const double *const *nodes = nullptr;
    double gamma = 0.0;
};
// Every refusal of ttx_set_integrand_pullback that needs no launch, in the order of include/ttx.h.  self, device, d, n: the pullback
// engine.  Returns TTX_OK or TTX_EINVAL with the message (which names the layer and the mode) in *msg.
inline int pb_check(const char *who, int m, const PbLayer *L, const void *self, int device, int d, const int *n, const double *const *ref, std::string *msg)
{
    char b[400];
    const auto bad = [&](const char *fmt, auto... a) { snprintf(b, sizeof b, fmt, a...); *msg = std::string(who) + ": " + b; return (int)TTX_EINVAL; };
    if (m < 1 || m > TTX_PULLBACK_MAX) return bad("%d layers (1..%d expected)", m, TTX_PULLBACK_MAX);
    if (!L) return bad("%s", "layer list missing");
    for (int t = 0; t < m; t++) {
        const PbLayer &y = L[t];
        if (!y.x) return bad("layer %d is null", t + 1);
        if (y.x == self) return bad("layer %d is the engine itself: its train is what the run writes", t + 1);
        if (!y.has_train) return bad("layer %d holds no tensor train", t + 1);
        if (!y.one_process) return bad("layer %d is spread over processes", t + 1);
        if (y.device != device) return bad("layer %d lives on device %d, the engine on device %d", t + 1, y.device, device);
        if (y.d != d) return bad("layer %d has %d modes, the engine %d", t + 1, y.d, d);
        for (int k = 0; k <= d; k++) if (y.r[k] < 1 || y.r[k] > TTX_PB_RMAX) return bad("layer %d: rank %d at bond %d (1..%d expected)", t + 1, y.r[k], k, TTX_PB_RMAX);
        if (y.r[0] != 1 || y.r[d] != 1) return bad("layer %d: boundary ranks are not 1", t + 1);
        for (int k = 0; k < d; k++) if (y.n[k] < 2) return bad("layer %d: mode %d has one index (every mode is drawn; held modes are not served)", t + 1, k + 1);
        if (!y.nodes) return bad("layer %d: node rows missing", t + 1);
        for (int k = 0; k < d; k++) {
            const std::string why = pb_bad_nodes(y.nodes[k], y.n[k], t >= 1);
            if (!why.empty()) return bad("layer %d, mode %d: the node row %s", t + 1, k + 1, why.c_str());
        }
        if (!(y.gamma >= 0.0) || !(y.gamma <= 1.7976931348623157e308)) return bad("layer %d: gamma is %g (finite and >= 0 expected)", t + 1, y.gamma);
        for (int s = 0; s < t; s++) {
            if (L[s].x != y.x) continue;
            bool same = L[s].gamma == y.gamma;
            for (int k = 0; same && k < d; k++) same = memcmp(L[s].nodes[k], y.nodes[k], sizeof(double) * (size_t)y.n[k]) == 0;
            if (!same) return bad("layers %d and %d are one engine with different nodes or gamma: both read one head (not served)", s + 1, t + 1);
        }
    }
    if (!ref) return bad("%s", "reference rows missing");
    for (int k = 0; k < d; k++) {
        const std::string why = pb_bad_ref(ref[k], n[k]);
        if (!why.empty()) return bad("mode %d: the reference row %s", k + 1, why.c_str());
    }
    return TTX_OK;
}
// the launch's LDS against what one workgroup can have, after pb_check: ldx and nmax over the layers
inline int pb_check_lds(const char *who, const PbPlan &p, int ldx, int nmax, int d, std::string *msg)
{
    if (!p.refused) return TTX_OK;
    char b[300];
    snprintf(b, sizeof b, "%s: one wave needs %zu bytes of LDS (largest rank %d rounded to four, largest layer mode %d, %d modes), a workgroup has %zu", who,
             sizeof(double) * p.per_wave, ldx, nmax, d, (size_t)TTX_LDS_WORK);
    *msg = b;
    return TTX_EINVAL;
}
