/*
 * tests/golden/oracle_var.c -- TEST INFRASTRUCTURE ONLY (fixture generator).
 *
 * The CPU oracle exports the Welford M2 of the solution only (oracle_solve_m2); its
 * stats_t also carries the gradient's (gM2, SampleStatistics::gradientM2,
 * walk_on_stars.h:744-877).  This file includes the oracle unmodified and adds one
 * export that runs its per-point path (solve_one's calls, in its order) and returns
 * the whole stats_t unmasked, next to the masked outputs oracle_solve_m2 writes.
 * Built by tests/golden/make_variance_golden.py with the flags of oracle/Makefile.
 */
#include "../../oracle/wos_oracle.c"

/* Per point i: p[i], grad[i*dim+k] as oracle_solve_m2 masks them; estimated[i];
 * sol_mean[i], g_mean[i*dim+k], n_sol[i], sol_m2[i], g_m2[i*dim+k] unmasked
 * (all 0 where the point is not estimated).  Single-threaded. */
int oracle_var_solve(const oracle_scene_desc *scene, const oracle_params *prm, const float *pts, int64_t n,
                     int64_t index_base, int64_t index_stride, float *p, float *grad, int32_t *estimated,
                     float *sol_mean, float *g_mean, int32_t *n_sol, float *sol_m2, float *g_m2)
{
    if (!scene || !prm || (n > 0 && !pts)) return -1;
    if (prm->n_walks < 1) return -2;
    scene_t sc;
    g_libm = prm->math_mode == 1;
    g_robust = prm->robust_float != 0;
    if (scene_build(&sc, scene)) { scene_free(&sc); return -3; }
    const int dim = sc.dim;
    pcount_t pc; memset(&pc, 0, sizeof(pc));
    for (int64_t i = 0; i < n; i++) {
        float x[3] = {0, 0, 0};
        for (int k = 0; k < dim; k++) x[k] = pts[i * dim + k];
        float dDist = dist_dirichlet(&sc, x, 0);
        float nDist = dist_neumann(&sc, x, 0);
        int inside = inside_domain(&sc, x);
        stats_t S; memset(&S, 0, sizeof(S));
        int est = 0;
        if (inside || sc.double_sided) {
            estimate_point(&sc, prm, x, (uint64_t)(index_base + i * index_stride), dDist, nDist, &S, &pc, NULL);
            est = 1;
        }
        float mask = prm->boundary_distance_mask;
        int maskP = fabsf(nDist) < mask;
        int maskG = (!inside && !sc.double_sided) || fabsf(nDist) < mask;
        p[i] = maskP ? 0.0f : (est ? S.solMean : 0.0f);
        estimated[i] = est;
        sol_mean[i] = S.solMean;
        n_sol[i] = S.nSol;
        sol_m2[i] = S.solM2;
        for (int k = 0; k < dim; k++) {
            grad[i * dim + k] = maskG ? 0.0f : (est ? S.gMean[k] : 0.0f);
            g_mean[i * dim + k] = S.gMean[k];
            g_m2[i * dim + k] = S.gM2[k];
        }
    }
    scene_free(&sc);
    return 0;
}
