// Host check of the three switches of the cluster launch entry in create_plan (ttcross_amd/csrc/ttx_create_plan.h) at the
// benchmark's C_64 configuration: TTX_CL_POWTAB, TTX_CL_WORD and TTX_CL_LISTS are on by default, each is turned off by =0 alone,
// and the lists are carried only where the kernel keeps them in LDS at all.  Prints the number of failed checks.
#include <cstdio>
#include <cstring>
#include "ttx_create_plan.h"
int main()
{
    int n[64]; double par[2 * 51 + 1];
    for (int k = 0; k < 64; k++) n[k] = 51;
    for (int j = 0; j < 51; j++) { par[j] = (j + 0.5) / 51; par[51 + j] = 1.0 / 51; }
    par[102] = 1.0;                                         // Ising C
    ttx_config cfg{};
    cfg.d = 63; cfg.n = n; cfg.maxrank = 32; cfg.pivoting = 2; cfg.fun_id = TTX_FUN_ISING; cfg.par = par; cfg.npar = 103; cfg.nproc = 8;
    cfg.world_size = 1; cfg.arith = TTX_ARITH_EXACT;
    DevCaps caps; caps.ncu = 256; caps.coop = true;
    const char *names[3] = {"TTX_CL_POWTAB", "TTX_CL_WORD", "TTX_CL_LISTS"};
    int bad = 0;
    for (int off = -1; off < 3; off++) {
        CreateEnv env = create_env_from([&](const char *name) -> const char * { return off >= 0 && !strcmp(name, names[off]) ? "0" : nullptr; });
        CreatePlan p = create_plan(cfg, false, env, caps);
        if (p.err != TTX_OK || !p.cluster_zkeep) bad++;
        if (p.cl_powtab != (off != 0) || p.cl_word != (off != 1) || p.cl_lists != (off != 2)) bad++;
    }
    CreateEnv one = create_env_from([&](const char *name) -> const char * { return !strcmp(name, "TTX_CL_LISTS") ? "1" : nullptr; });
    if (!create_plan(cfg, false, one, caps).cl_lists) bad++;
    cfg.nproc = 1; cfg.maxrank = 64;                        // 62 own bonds at rank 64: the lists do not fit the LDS, nothing to carry
    CreatePlan big = create_plan(cfg, false, CreateEnv(), caps);
    if (big.err != TTX_OK || big.cluster_zkeep || big.cl_lists || !big.cl_word || !big.cl_powtab) bad++;
    printf("%d\n", bad);
    return bad != 0;
}
