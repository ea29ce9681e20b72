// Pose-graph marginal covariances (pgcov.inc, a part of posegraph.hip; include/mloam_hip.h section (f18)): what exists once for the kernels (__host__ __device__), for the host side of the
// entry and for a stand-alone host program that runs it under a sanitizer (tests/host/pg_marg_main.cpp) -- the launch plan, the buffer sizes, the window indexing of
// the band's selected inversion, and the conversion of a block from the solver's tangent to the keyframe store's convention.
//
// The conversion. The solver's tangent is pg_plus's (pg_host.hpp): delta = [d_r, d_t]; the quaternion is multiplied FROM THE LEFT by (cos |d_r|, sin |d_r| d_r / |d_r|),
// a turn by the angle 2 |d_r| about d_r, and d_t is added to t. The keyframe store's covariances are over the left perturbation T = exp(xi^) T_bar with
// xi = [rho, phi] (associate_uct.hpp: evalPointUncertainty's G = [I, -[R p + t]x]). To first order exp(xi^) T_bar = (exp(phi^) R_bar, t_bar + phi x t_bar + rho), so
//   phi = 2 d_r                       (the left turn, as an axis-angle vector)
//   rho = d_t - phi x t_bar = d_t + 2 [t_bar]x d_r
// i.e. xi = A delta with A = [[2 [t]x, I], [2 I, 0]] -- rows rho, phi; columns rotation, translation; t the keyframe's stored translation -- and the block becomes
// A Sigma A^T. The next term of both sides is quadratic in delta (tests/test_pg_marg_cases.py bounds it).
// Translation units that include this header are compiled with -ffp-contract=off.
#pragma once
#include "pg_host.hpp"

namespace mlh {

// ---- the launch plan. M keyframes, L loop edges (m = 6 L):
//   M == 1: begin, linearise, state record, tail                                                            4 launches
//   else:   begin, linearise, state record, assemble (raw), unit scaling, band factor, forward, Gram,
//           the dense stage (1 launch for L <= PG_MAX_LOOPS, 3 ceil(6 L / 64) beyond: pg_dense_launches),
//           factor pack, selected inversion, Z = L^-T Y, Q = L_c^-1 Z^T, tail                             13 + dense
constexpr int PGM_FIXED_LAUNCHES = 13;
inline int pgm_launches(int M, int L)
{
    if (M <= 1) return 4;
    return PGM_FIXED_LAUNCHES + (L <= PG_MAX_LOOPS ? 1 : pg_dense_launches(6 * L));
}

// ---- the buffers beyond an optimise's, in doubles. mp = 6 L rounded up to the panel width.
inline size_t pgm_panel_cols(int L) { return size_t((6 * L + PG_PANEL - 1) / PG_PANEL) * PG_PANEL; }
// both forms, 36 doubles per keyframe each: the local form first
inline size_t pgm_out_doubles(int M) { return size_t(2) * 36 * size_t(M); }
// the band's selected inverse (NB x 5 blocks of 36, as the factor's rows are stored) and, for L <= PG_MAX_LOOPS, the dense factor transposed (mp x mp; beyond, the
// blocked stage's own factor is used in place)
inline size_t pgm_band_doubles(int M) { return size_t(M > 1 ? M - 1 : 0) * PG_SLOTS * 36; }
inline size_t pgm_factor_doubles(int L) { return L <= PG_MAX_LOOPS ? pgm_panel_cols(L) * pgm_panel_cols(L) : 0; }
inline size_t pgm_factor_offset(int M) { return ((pgm_band_doubles(M) + 15) / 16) * 16; }          // the packed factor behind the band's inverse, 128-byte aligned
inline size_t pgm_work_doubles(int M, int L) { return pgm_factor_offset(M) + pgm_factor_doubles(L) + 16; }

// ---- the selected inversion's window: block (i, k) of B^-1, |i - k| <= 4, lives in slot (i mod 5, k mod 5) of a 5 x 5-block circular window, BOTH triangles (the
// transpose in the mirrored slot). Step j (from NB - 1 down) reads the slots of i, k in j + 1 .. j + 4 and writes row and column j mod 5 -- which held block row /
// column j + 5, read for the last time at step j + 1.
MLH_PG_HD int pgm_win_slot(int i, int k) { return (i % 5) * 5 + k % 5; }

// ---- the conversion: out = A S A^T for the symmetric block S (6 x 6 row-major over [rotation, translation]) and the stored translation t. The lower triangle is
// computed, the upper copied: symmetric to the bit.
MLH_PG_HD void pgm_store_A(const double t[3], double A[36])
{
    for (int c = 0; c < 36; ++c) A[c] = 0.0;
    // rho rows: 2 [t]x over the rotation columns, I over the translation columns
    A[0 * 6 + 1] = -2.0 * t[2]; A[0 * 6 + 2] = 2.0 * t[1];
    A[1 * 6 + 0] = 2.0 * t[2];  A[1 * 6 + 2] = -2.0 * t[0];
    A[2 * 6 + 0] = -2.0 * t[1]; A[2 * 6 + 1] = 2.0 * t[0];
    for (int c = 0; c < 3; ++c) { A[c * 6 + 3 + c] = 1.0; A[(3 + c) * 6 + c] = 2.0; }
}
MLH_PG_HD void pgm_to_store(const double S[36], const double t[3], double out[36])
{
    double A[36], AS[36];
    pgm_store_A(t, A);
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
            for (int q = 0; q < 6; ++q) v += A[a * 6 + q] * S[q * 6 + c];
            AS[a * 6 + c] = v;
        }
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c <= a; ++c) {
            double v = 0.0;
            for (int q = 0; q < 6; ++q) v += AS[a * 6 + q] * A[c * 6 + q];
            out[a * 6 + c] = v; out[c * 6 + a] = v;
        }
}

}  // namespace mlh
