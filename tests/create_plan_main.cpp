// Stand-alone check of ttcross_amd/csrc/ttx_create_plan.h (host code only): prints the plan of engine creation for a list of
// configurations, one line each (tests/test_create_plan_cpu.py holds the expected lines), then checks every plan of a grid of
// configurations for the conditions the kernels rely on.  Built plain and with -fsanitize=address,undefined by that test.
#include "ttx_create_plan.h"

#include <cstdio>
#include <map>
#include <string>
#include <utility>
#include <vector>

// one configuration: an integrand at a shape, the environment, the device's figures, the occupancy the runtime would report
struct Case {
    std::string name;
    int fun = TTX_FUN_ISING, ising_id = 1;
    int d = 6, n = 9, r = 4, piv = 2, nproc = 1, W = 1, wrank = 0, arith = TTX_ARITH_EXACT;
    bool nofun = false;
    std::map<std::string, std::string> env;
    int ncu = 256, occ = 8; bool coop = true;
    std::vector<int32_t> modes, mybonds;        // where not empty: the mode sizes instead of n everywhere, own(0:nproc)
    int node = -1; double node_value = 0.0;     // one node of par set to a value
    int naux_short = 0; double det = 1.0;       // mvn: aux shorter by this many; its determinant
};
// the caller's arrays of a case, alive as long as the configuration is in use
struct Config {
    std::vector<int32_t> n, own;
    std::vector<double> par, aux;
    ttx_config cfg{};
    Config(const Config &) = delete;            // cfg points into the vectors
    explicit Config(const Case &c)
    {
        n = c.modes.empty() ? std::vector<int32_t>(c.d, c.n) : c.modes;
        const int n0 = n[0];
        if (c.fun == TTX_FUN_ISING) {
            par.assign(2 * n0 + 1, 1.0 / n0);
            for (int j = 0; j < n0; j++) par[j] = (j + 0.5) / n0;
            par[2 * n0] = c.ising_id;
        } else if (c.fun == TTX_FUN_STDNORM || c.fun == TTX_FUN_MVN) {
            par.assign(n0, 0.0);
            for (int j = 0; j < n0; j++) par[j] = -5.0 + 10.0 * (j + 0.5) / n0;
        }
        if (c.node >= 0) par[c.node] = c.node_value;
        if (c.fun == TTX_FUN_MVN) {             // mu = 0, inverse covariance = identity, determinant
            aux.assign((size_t)c.d + (size_t)c.d * c.d + 1, 0.0);
            for (int i = 0; i < c.d; i++) aux[c.d + i + (size_t)c.d * i] = 1.0;
            aux.back() = c.det;
        }
        own = c.mybonds;
        cfg.d = c.d; cfg.n = n.data(); cfg.fun_id = c.fun;
        cfg.par = par.empty() ? nullptr : par.data(); cfg.npar = (int32_t)par.size();
        cfg.aux = aux.empty() ? nullptr : aux.data(); cfg.naux = (int32_t)aux.size() - c.naux_short;
        cfg.accuracy = 1e-10; cfg.maxrank = c.r; cfg.pivoting = c.piv;
        cfg.nproc = c.nproc; cfg.mybonds = own.empty() ? nullptr : own.data();
        cfg.world_rank = c.wrank; cfg.world_size = c.W; cfg.arith = c.arith;
    }
};

static CreatePlan plan_of(const Case &c, const Config &k)
{
    const CreateEnv env = create_env_from([&](const char *name) -> const char * {
        const auto it = c.env.find(name);
        return it == c.env.end() ? nullptr : it->second.c_str();
    });
    DevCaps caps; caps.ncu = c.ncu; caps.coop = c.coop;
    CreatePlan p = create_plan(k.cfg, c.nofun, env, caps);
    if (!p.err) create_admit(p, c.occ);
    return p;
}

static void print_plan(const Case &c)
{
    const Config k(c);
    const CreatePlan p = plan_of(c, k);
    printf("%s ->", c.name.c_str());
    if (p.err) { printf(" error %d: %s\n", p.err, p.errtext.c_str()); return; }
    printf(" W=%d nproc=%d G=%d g0=%d nbmax=%d NC=%d NM=%d mode=%d H=%d own=", p.W, p.nproc, p.G, p.g0, p.nbmax, p.NC, p.NM, p.mode, p.H);
    for (size_t g = 0; g < p.own.size(); g++) printf("%s%d", g ? "," : "", p.own[g]);
    printf(" SS=%zu SW=%zu CS=%zu nfb=%d XD=%zu IOFF=%zu MSZ=%zu QB=%zu SB=%zu HS=%zu slot_dev=%d nn=%d snum=%d lot_max=%d lot_nb=%d de_npair=%d de_slots=%d FD=%d cdf=%d norm=%.17g",
           p.SS, p.SW, p.CS, p.nfb, p.XD, p.IOFF, p.MSZ, p.QB, p.SB, p.HS, (int)(p.slots == SLOTS_DEVICE), p.nn, p.snum, p.nlotmax, p.lot_nb, p.de_npair,
           p.de_slots, p.FD, p.cdf_kmax, p.mvn_norm);
    printf(" | want_fast=%d unit=%d arith=%d fpersist=%d de_unit=%d de_cut=%d de_v2=%d de_v5=%d de_team=%d/%d/%d fault=%d lot_point=%d lot_wave=%d lot_rows=%d"
           " mvn_v2=%d bnd_wave=%d lotc=%d pfull=%d fp_mfma=%d/%d qscr=%d half_vals=%d lot_vals=%d fast_cap=%d fused=%d cluster=%d var=%d ldsinv=%d zkeep=%d coop=%d",
           (int)p.want_fast, (int)p.unit_nodes, p.arith, p.fpersist, p.de_unit, p.de_cut, p.de_v2, p.de_v5, p.de_team, p.de_team_units, p.de_team6_units,
           p.de_test_fault, p.de_lot_point, p.lot_wave, p.lot_rows, p.mvn_v2, p.bnd_wave, (int)p.lot_cand, (int)p.pfull, p.fp_mfma, p.fp_tiles, (int)p.qscr,
           p.half_vals, p.lot_vals, p.fast_cap, p.fused, p.cluster, p.cluster_var, p.cluster_ldsinv, p.cluster_zkeep, p.cluster_coop);
    printf(" | lds par=%zu half=%zu lot=%zu fused=%zu cluster=%zu de=%zu det=%zu det6=%zu de5=%zu der=%zu mvn=%zu\n",
           p.lds_par, p.lds_half, p.lds_lot, p.lds_fused, p.lds_cluster, p.lds_de, p.lds_det, p.lds_det6, p.lds_de5, p.lds_der, p.lds_mvn);
}

static int bad = 0;
static long refused = 0;        // plans of the grid that are refusals
#define CHECK(c_) do { if (!(c_)) { if (bad++ < 20) printf("FAILED %s: %s\n", c.name.c_str(), #c_); } } while (0)
static void check_plan(const Case &c, const Config &k)
{
    const CreatePlan p = plan_of(c, k);
    refused++;
    if (p.err) {        // the two refusals a valid call of the grid can meet
        // mvn from 387 dimensions on: (2 pi)^d alone is beyond the double range, whatever the determinant
        if (c.fun == TTX_FUN_MVN && c.d >= 387) { CHECK(p.err == TTX_EINVAL && p.errtext.compare(0, 29, "ttx_create: mvn normalisation") == 0); return; }
        CHECK(p.err == TTX_EINVAL && p.errtext == "problem too large for LDS staging (d*maxrank)");
        const size_t VS = ((c.d + 7) & ~7) + 8;
        CHECK(sizeof(short) * 2 * c.r * VS > TTX_LDS_LOTTERY / 2);         // the index rows alone are past half the lottery's budget
        return;
    }
    refused--;
    // every LDS size of a kernel the plan lets run fits a workgroup
    CHECK(p.lds_par <= TTX_LDS_DEVICE && p.lds_half <= TTX_LDS_DEVICE && p.lds_lot <= TTX_LDS_DEVICE);
    if (p.de_v2) CHECK(p.lds_de <= TTX_LDS_DEVICE);
    if (p.de_team) CHECK(p.lds_det <= TTX_LDS_DEVICE && p.lds_det6 <= TTX_LDS_DEVICE);
    if (p.de_v5) CHECK(p.lds_de5 <= TTX_LDS_DEVICE);
    if (p.lot_wave || (p.isDE && p.bnd_wave && p.de_npair)) CHECK(p.lds_der <= TTX_LDS_DEVICE);
    if (p.mvn_v2) CHECK(p.lds_mvn <= TTX_LDS_DEVICE);
    if (p.fused) CHECK(p.lds_fused <= TTX_LDS_DEVICE);
    if (p.cluster) CHECK(p.lds_cluster <= TTX_LDS_DEVICE);
    CHECK(!p.de_team || p.de_v2); CHECK(!p.de_v5 || p.de_v2); CHECK(!p.lot_wave || p.de_v2);
    CHECK(!p.de_v2 || p.de_slots <= TTX_MAXPART); CHECK(!p.mvn_v2 || p.de_slots <= TTX_MAXPART);
    CHECK(p.cluster < 2 || p.G * p.cluster <= c.ncu);
    CHECK(p.cluster != 1);                                                  // a cluster has at least two workgroups
    CHECK(!(p.fused && p.cluster));
    CHECK(p.lot_nb >= 1 && (p.lot_nb == 1 || p.lot_nb * 64 >= p.nlotmax));
    CHECK(!p.lot_cand || p.isDE || p.mvn_v2);
    CHECK(p.arith == 0 || p.want_fast);
}

int main()
{
    std::vector<Case> list;
    auto add = [&](const char *name, Case c) { c.name = name; list.push_back(c); return c; };
    auto with_env = [](Case c, std::initializer_list<std::pair<const char *, const char *>> kv) { for (auto &e : kv) c.env[e.first] = e.second; return c; };
    // ---- Ising C, d=6 n=9 r=4 piv=2 ----
    Case C; C.fun = TTX_FUN_ISING; C.ising_id = 1;
    add("C default", C);
    { Case c = C; c.occ = 0; add("C occupancy 0", c); }
    { Case c = C; c.ncu = 32; c.occ = 4; add("C 32 CUs", c); }
    { Case c = C; c.ncu = 32; c.occ = 3; add("C 32 CUs occupancy 3", c); }
    add("C SWEEP=chain", with_env(C, {{"TTX_SWEEP", "chain"}}));
    add("C SWEEP=fused", with_env(C, {{"TTX_SWEEP", "fused"}}));
    add("C SWEEP=cluster", with_env(C, {{"TTX_SWEEP", "cluster"}}));
    { Case c = with_env(C, {{"TTX_SWEEP", "cluster"}}); c.occ = 0; add("C SWEEP=cluster occupancy 0", c); }
    add("C SWEEP=bogus", with_env(C, {{"TTX_SWEEP", "bogus"}}));
    add("C CL_PAD=0", with_env(C, {{"TTX_CL_PAD", "0"}}));
    add("C CL_PAD=1", with_env(C, {{"TTX_CL_PAD", "1"}}));
    add("C CL_PAD=yes", with_env(C, {{"TTX_CL_PAD", "yes"}}));
    { Case c = C; c.node = 3; c.node_value = 1.5; add("C node 1.5", c); }
    { Case c = C; c.arith = TTX_ARITH_FAST; add("C fast", c); }
    { Case c = C; c.arith = TTX_ARITH_FAST; c.occ = 0; add("C fast occupancy 0", c); }
    add("C ARITH=fast", with_env(C, {{"TTX_ARITH", "fast"}}));
    add("C ARITH=quick", with_env(C, {{"TTX_ARITH", "quick"}}));
    { Case c = C; c.arith = 2; add("C arith 2", c); }
    { Case c = C; c.r = 65; add("C r=65", c); }
    { Case c = C; c.r = 64; add("C r=64", c); }
    { Case c = C; c.d = 12; c.nproc = 2; add("C d=12 nproc=2", c); }
    { Case c = with_env(C, {{"TTX_SWEEP", "fused"}}); c.d = 12; c.nproc = 2; add("C d=12 nproc=2 SWEEP=fused", c); }
    { Case c = C; c.d = 12; c.nproc = 5; add("C d=12 nproc=5", c); }
    { Case c = C; c.d = 12; c.nproc = 5; c.ncu = 32; add("C d=12 nproc=5 32 CUs", c); }
    { Case c = C; c.d = 12; c.nproc = 4; c.W = 2; c.wrank = 1; add("C d=12 nproc=4 rank 1 of 2", c); }
    { Case c = C; c.d = 40; c.nproc = 20; add("C d=40 nproc=20 (NB shrinks)", c); }
    { Case c = C; c.d = 80; c.nproc = 70; add("C d=80 nproc=70 (no cluster)", c); }
    add("C CLUSTER_NB=3 COOP=1 TEST_ABORT=2", with_env(C, {{"TTX_CLUSTER_NB", "3"}, {"TTX_CLUSTER_COOP", "1"}, {"TTX_CLUSTER_TEST_ABORT", "2"}}));
    { Case c = with_env(C, {{"TTX_CLUSTER_COOP", "1"}}); c.coop = false; add("C COOP=1 without the attribute", c); }
    { Case c = C; c.piv = -1; add("C piv=-1", c); }
    { Case c = with_env(C, {{"TTX_FULLPIV", "mfma"}}); c.piv = -1; add("C piv=-1 FULLPIV=mfma", c); }
    { Case c = with_env(C, {{"TTX_FULLPIV", "mfma"}}); c.piv = -1; c.r = 65; add("C piv=-1 FULLPIV=mfma r=65", c); }
    { Case c = C; c.piv = 0; add("C piv=0", c); }
    // ---- Ising D, d=45 n=9 r=6 piv=2 ----
    Case Dd; Dd.fun = TTX_FUN_ISING; Dd.ising_id = 2; Dd.d = 45; Dd.n = 9; Dd.r = 6;
    add("D default", Dd);
    add("D LOT_POINT=0", with_env(Dd, {{"TTX_DE_LOT_POINT", "0"}}));
    add("D LANE=1", with_env(Dd, {{"TTX_DE_LANE", "1"}}));
    add("D V2=0", with_env(Dd, {{"TTX_DE_V2", "0"}}));
    add("D CUT=0", with_env(Dd, {{"TTX_DE_CUT", "0"}}));
    add("D CUT=0 FASTDIV=0", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_FASTDIV", "0"}}));
    add("D CUT=0 LOTTERY_ROWS=2", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_LOTTERY_ROWS", "2"}}));
    add("D CUT=0 LOTTERY_WAVE=0", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_LOTTERY_WAVE", "0"}}));
    add("D CUT=0 V5=1", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_V5", "1"}}));
    add("D CUT=0 V2=0", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_V2", "0"}}));
    add("D CUT=0 TEAM=0", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_TEAM", "0"}}));
    add("D CUT=0 TEAM_UNITS=1000000", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_TEAM_UNITS", "1000000"}}));
    add("D CUT=0 TEAM_UNITS=0 TEAM6_UNITS=1000000", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_TEAM_UNITS", "0"}, {"TTX_DE_TEAM6_UNITS", "1000000"}}));
    add("D TABLES=0", with_env(Dd, {{"TTX_DE_TABLES", "0"}}));
    add("D CUT=0 TEST_FAULT=2 LOTTERY_NB=1", with_env(Dd, {{"TTX_DE_CUT", "0"}, {"TTX_DE_TEST_FAULT", "2"}, {"TTX_LOTTERY_NB", "1"}}));
    { Case c = Dd; c.arith = TTX_ARITH_FAST; add("D fast", c); }
    { Case c = Dd; c.node = 3; c.node_value = 1.5; add("D node 1.5", c); }
    { Case c = Dd; c.node = 3; c.node_value = 1.5; c.arith = TTX_ARITH_FAST; add("D node 1.5 fast", c); }
    { Case c = Dd; c.d = 160; add("D d=160", c); }
    { Case c = Dd; c.d = 161; add("D d=161", c); }
    { Case c = Dd; c.d = 3; c.n = 257; c.r = 128; add("D d=3 n=257 r=128", c); }
    { Case c = Dd; c.piv = -1; add("D piv=-1", c); }
    { Case c = Dd; c.ising_id = 3; c.nproc = 3; add("E nproc=3", c); }
    // ---- mvn, d=6 n=9 r=4 ----
    Case M; M.fun = TTX_FUN_MVN;
    add("mvn default", M);
    add("mvn MVN_V2=0", with_env(M, {{"TTX_MVN_V2", "0"}}));
    { Case c = M; c.arith = TTX_ARITH_FAST; add("mvn fast", c); }
    { Case c = with_env(M, {{"TTX_FAST_PERSIST", "0"}}); c.arith = TTX_ARITH_FAST; add("mvn fast FAST_PERSIST=0", c); }
    { Case c = M; c.naux_short = 1; add("mvn aux short", c); }
    { Case c = M; c.det = 1e308; add("mvn det 1e308", c); }
    { Case c = M; c.det = -1.0; add("mvn det -1", c); }
    { Case c = M; c.d = 513; add("mvn d=513", c); }
    { Case c = M; c.d = 512; add("mvn d=512", c); }
    { Case c = M; c.piv = -1; add("mvn piv=-1", c); }
    // ---- stdnorm, n=2 r=128 piv=2 ----
    Case S; S.fun = TTX_FUN_STDNORM; S.n = 2; S.r = 128;
    { Case c = S; c.d = 200; add("stdnorm d=200 n=2 r=128", c); }
    { Case c = S; c.d = 240; add("stdnorm d=240 n=2 r=128", c); }
    { Case c = S; c.d = 6; c.n = 9; c.r = 4; add("stdnorm d=6 n=9 r=4", c); }
    // ---- two-pass integrands, d=4 n=5 r=3 ----
    Case Hh; Hh.d = 4; Hh.n = 5; Hh.r = 3;
    { Case c = Hh; c.fun = TTX_FUN_HOST; add("host", c); }
    { Case c = Hh; c.fun = TTX_FUN_HOST; c.modes = {5, 3, 300, 4}; c.nproc = 3; add("host modes 5,3,300,4 nproc=3", c); }
    { Case c = Hh; c.fun = TTX_FUN_COSCOEFF; add("coscoeff", c); }
    { Case c = Hh; c.fun = TTX_FUN_DEVICE; add("device", c); }
    { Case c = Hh; c.fun = TTX_FUN_TRAINS; add("trains", c); }
    { Case c = Hh; c.fun = TTX_FUN_TRAINS; c.arith = TTX_ARITH_FAST; add("trains fast", c); }
    { Case c = Hh; c.fun = 0; c.nofun = true; add("nofun", c); }
    { Case c = Hh; c.fun = 0; c.nofun = true; c.arith = TTX_ARITH_FAST; add("nofun fast", c); }
    // ---- refusals ----
    { Case c = C; c.nproc = 2; c.mybonds = {1, 1, 6}; add("mybonds empty group", c); }
    { Case c = C; c.nproc = 2; c.mybonds = {1, 3, 5}; add("mybonds short of d", c); }
    { Case c = C; c.nproc = 2; c.mybonds = {2, 4, 6}; add("mybonds not from 1", c); }
    { Case c = C; c.nproc = 2; c.mybonds = {1, 2, 6}; add("mybonds 1,2,6", c); }
    { Case c = C; c.modes = {9, 9, 0, 9, 9, 9}; add("a mode of 0", c); }
    { Case c = C; c.fun = TTX_FUN_HOST; c.modes = {9, 9, 32001, 9, 9, 9}; add("a mode of 32001", c); }
    { Case c = C; c.fun = TTX_FUN_HOST; c.modes = {9, 9, 32000, 9, 9, 9}; c.r = 5; add("maxrank*n too large", c); }
    { Case c = C; c.fun = TTX_FUN_HOST; c.modes = {9, 9, 1024, 9, 9, 9}; c.r = 128; add("maxrank*n at the limit", c); }
    for (const Case &c : list) print_plan(c);

    // ---- the grid ----
    const int ds[] = {2, 3, 8, 64, 160, 161, 256, 512}, ns[] = {1, 2, 9, 64, 65, 257}, rs[] = {1, 4, 64, 65, 128}, pivs[] = {-1, 0, 2};
    struct Fun { int fun, ising_id; const char *name; };
    const Fun funs[] = {{TTX_FUN_ISING, 1, "C"}, {TTX_FUN_ISING, 2, "D"}, {TTX_FUN_STDNORM, 0, "stdnorm"}, {TTX_FUN_MVN, 0, "mvn"}, {TTX_FUN_HOST, 0, "host"}, {TTX_FUN_COSCOEFF, 0, "coscoeff"}};
    // the switches that move a limit: nothing set; the full Ising D/E tables; every optional variant off
    const std::map<std::string, std::string> envs[] = {
        {}, {{"TTX_DE_CUT", "0"}, {"TTX_DE_V5", "1"}, {"TTX_FULLPIV", "mfma"}},
        {{"TTX_DE_V2", "0"}, {"TTX_MVN_V2", "0"}, {"TTX_SWEEP", "chain"}, {"TTX_LOTTERY_NB", "1"}}};
    long count = 0;
    for (int d : ds) for (int n : ns) for (int r : rs) for (const Fun &f : funs) {
        Case c; c.fun = f.fun; c.ising_id = f.ising_id; c.d = d; c.n = n; c.r = r;
        Config k(c);                            // the arrays do not depend on what varies below
        for (int piv : pivs) {
            count++;
            for (size_t e = 0; e < sizeof envs / sizeof envs[0]; e++) for (int fast = 0; fast < 2; fast++) for (int dev = 0; dev < 3; dev++) {
                c.piv = piv; c.env = envs[e]; c.arith = fast; c.nproc = (dev == 2 && d > 20) ? 20 : 1;
                c.ncu = dev == 1 ? 32 : 256; c.occ = dev == 1 ? 0 : 8;
                c.name = std::string(f.name) + " d=" + std::to_string(d) + " n=" + std::to_string(n) + " r=" + std::to_string(r) + " piv=" + std::to_string(piv) +
                         " env " + std::to_string(e) + " fast " + std::to_string(fast) + " device " + std::to_string(dev);
                k.cfg.pivoting = piv; k.cfg.arith = fast; k.cfg.nproc = c.nproc;
                check_plan(c, k);
            }
        }
    }
    if (bad) printf("create plan: %d checks FAILED\n", bad);
    else printf("create plan: ok (%ld configurations, %ld of their %ld plans refusals)\n", count, refused, count * 18);
    return bad != 0;
}
