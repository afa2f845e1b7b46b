// Host check of the stretch between two sweeps: who packs which part at the exit of a cluster launch (cl_pack_block of
// ttcross_amd/csrc/ttx_cluster_rules.h) for every cluster size 1 .. TTX_CLMAX -- every part by exactly one workgroup of the cluster,
// red[] with the right-going message on workgroup 0, the left-going message on workgroup 1 where there is one and the split is on --
// and the three switches in create_plan (ttx_create_plan.h) at the benchmark's C_64 configuration: TTX_TAIL_EVENT (kernel by
// default, marker on request, anything else refused), TTX_TAIL_LEAN and TTX_CL_PACK2 (on by default, each turned off
// by =0 alone).  Prints "<failed checks> <checks>".
#include <cstdio>
#include <cstring>
#include "ttx_create_plan.h"
#include "ttx_cluster_rules.h"

static int bad = 0, nchk = 0;
#define CHECK(c) do { nchk++; if (!(c)) { bad++; fprintf(stderr, "line %d: %s\n", __LINE__, #c); } } while (0)

int main()
{
    for (int NB = 1; NB <= TTX_CLMAX; NB++)
        for (int split = 0; split < 2; split++) {
            for (int part = CL_PACK_RIGHT; part <= CL_PACK_LEFT; part++) {
                int packers = 0;
                for (int cb = 0; cb < NB; cb++) packers += cl_pack_block(part, NB, split != 0) == cb;
                CHECK(packers == 1);                                        // exactly once, by a workgroup the cluster has
            }
            CHECK(cl_pack_block(CL_PACK_RIGHT, NB, split != 0) == 0);       // red[] reads what workgroup 0 writes
            CHECK(cl_pack_block(CL_PACK_LEFT, NB, split != 0) == ((split && NB >= 2) ? 1 : 0));
        }

    int n[64]; double par[2 * 51 + 1];
    for (int k = 0; k < 64; k++) n[k] = 51;
    for (int j = 0; j < 51; j++) { par[j] = (j + 0.5) / 51; par[51 + j] = 1.0 / 51; }
    par[102] = 1.0;                                         // Ising C
    ttx_config cfg{};
    cfg.d = 63; cfg.n = n; cfg.maxrank = 32; cfg.pivoting = 2; cfg.fun_id = TTX_FUN_ISING; cfg.par = par; cfg.npar = 103; cfg.nproc = 8;
    cfg.world_size = 1; cfg.arith = TTX_ARITH_EXACT;
    DevCaps caps; caps.ncu = 256; caps.coop = true;
    const char *names[2] = {"TTX_TAIL_LEAN", "TTX_CL_PACK2"};
    for (int off = -1; off < 2; off++)
        for (int one = 0; one < 2; one++) {                 // the others unset, or set to 1
            CreateEnv env = create_env_from([&](const char *name) -> const char * {
                for (int k = 0; k < 2; k++) if (!strcmp(name, names[k])) return k == off ? "0" : one ? "1" : nullptr;
                return nullptr;
            });
            CreatePlan p = create_plan(cfg, false, env, caps);
            CHECK(p.err == TTX_OK);
            CHECK(p.tail_lean == (off != 0)); CHECK(p.cl_pack2 == (off != 1));
            CHECK(p.tail_event_kernel);
        }
    const char *words[4] = {nullptr, "kernel", "marker", "signal"};
    for (int w = 0; w < 4; w++) {
        CreateEnv env = create_env_from([&](const char *name) -> const char * { return !strcmp(name, "TTX_TAIL_EVENT") ? words[w] : nullptr; });
        CreatePlan p = create_plan(cfg, false, env, caps);
        if (w == 3) { CHECK(p.err == TTX_EINVAL); CHECK(p.errtext.find("TTX_TAIL_EVENT") != std::string::npos); continue; }
        CHECK(p.err == TTX_OK);
        CHECK(p.tail_event_kernel == (w != 2));
        CHECK(p.tail_lean && p.cl_pack2);
    }
    printf("%d %d\n", bad, nchk);
    return bad != 0;
}
