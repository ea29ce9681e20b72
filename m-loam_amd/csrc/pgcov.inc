// Pose-graph marginal covariances on the device (gfx950): include/mloam_hip.h, section (f18), has the contract; pg_marg_host.hpp the plan and the conversion. Included
// by posegraph.hip inside its namespace: everything up to the dense factor is that file's own kernels, run on the UNDAMPED system (S = 1, diag = 0 fed to
// pg_band_entry: (1 * v) * 1 + 0 / radius is v to the bit).
// With H = B + W^T W (B the sequential edges' block band, W the 6 L rows of the loop edges' corrected Jacobians), B = L L^T, Y = L^-1 W^T and C = I + Y^T Y = L_c L_c^T,
// Woodbury gives H^-1 = B^-1 - Z C^-1 Z^T with Z = L^-T Y. Only the 6 x 6 diagonal blocks are formed; nothing of size n x n exists.
//   pgm_unit_kernel     S = 1, diag = 0, S g = 0 (the right-hand side column of Y is carried along as zeros)
//   pgm_pack_kernel     the dense factor as ONE layout for what follows: U[j][r] = L_c[r][j], r >= j (the contraction index slow, as the blocked stage stores it).
//                       L <= 128: pg_dense_kernel's row-major factor transposed into a buffer of the marginals' own, identity in the padding; beyond: the blocked
//                       stage's diagonal factors (P.Dg) copied over the stale diagonal tiles of P.C, which is then that layout in place
//   pgm_selinv_kernel   the blocks (i, j), |i - j| <= 4, of B^-1 from L by Takahashi's recursion, from the last block column to the first: with G_kj = L_kj L_jj^-1,
//                       Sigma_ij = -sum_k Sigma_ik G_kj (i = j + 1 .. j + 4) and Sigma_jj = L_jj^-T L_jj^-1 - sum_k Sigma_jk G_kj, k = j + 1 .. j + 4. One
//                       workgroup, a 5 x 5-block circular window in LDS (pg_marg_host.hpp: pgm_win_slot), L's next block column fetched while a step computes: the
//                       mirror of pg_factor_kernel
//   pgm_zback_kernel    Z = L^-T Y in place: one lane per column, one sweep from the last block to the first, L's block column staged once per step in LDS
//                       (double-buffered) for all lanes: the mirror of pg_forward_kernel
//   pgm_trsm_kernel     Q = L_c^-1 Z^T in place -- row i of the Y buffer is one right-hand side, so Q^T = Z L_c^-T: a workgroup owns 64 rows and walks the 64-wide
//                       panels left to right with no other workgroup to wait for; panel k's update (minus the products with ALL earlier panels, j ascending in one
//                       accumulator chain) on v_mfma_f64_16x16x4_f64, a wavefront per 16 rows x 64 columns, then the 64 x 64 triangle solved scalar with 16 unknowns
//                       per thread in registers, one barrier per column (pg_cpanel_kernel's shape). O(n m^2): where the time goes at large L
//   pgm_tail_kernel     a wavefront per keyframe: the block's 6 x 6 Gram of its six rows of Q (lanes stride the columns, a fixed xor-tree), Sigma_bb =
//                       [B^-1]_bb - Gram, lower triangle computed and mirrored; both forms written (the store form: pgm_to_store). Block `first`: zeros
// Every sum has one order; no atomics; every kernel returns at once when a pivot of B or C was not positive (the tail then writes nothing).

struct PgMarg {
    double *Sband;               // [B^-1]_(j + d, j) at (j * 5 + d) * 36, d = 0 .. 4
    double *U;                   // the dense factor, transposed: U[j * ldu + r] = L_c[r][j]
    double *out;                 // 36 M doubles of the local form, then 36 M of the store form
    int ldu, mp;                 // mp = m rounded up to the panel width
};

__global__ __launch_bounds__(PG_TPB) void pgm_unit_kernel(PgDev P)
{
    const int i = blockIdx.x * PG_TPB + threadIdx.x;
    if (i >= P.n) return;
    P.S[i] = 1.0; P.diag[i] = 0.0; P.gs[i] = 0.0;
}

__global__ __launch_bounds__(PG_TPB) void pgm_pack_kernel(PgDev P, PgMarg Q)
{
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int m = P.m;
    if (P.T == 0) {
        const size_t total = size_t(Q.mp) * Q.mp;
        for (size_t idx = size_t(blockIdx.x) * PG_TPB + threadIdx.x; idx < total; idx += size_t(gridDim.x) * PG_TPB) {
            const int j = int(idx / size_t(Q.mp)), r = int(idx % size_t(Q.mp));
            Q.U[idx] = (r < m && r >= j) ? P.C[size_t(r) * m + j] : (r == j ? 1.0 : 0.0);
        }
        return;
    }
    for (int k = int(blockIdx.x); k < P.T; k += int(gridDim.x)) {
        const double *D = P.Dg + size_t(k) * PG_PANEL * PG_PANEL;
        for (int idx = threadIdx.x; idx < PG_PANEL * PG_PANEL; idx += PG_TPB) {
            const int c = idx >> 6, r = idx & 63;
            P.C[(size_t(k) * PG_PANEL + c) * P.ld + size_t(k) * PG_PANEL + r] = r >= c ? D[idx] : 0.0;
        }
    }
}

__global__ __launch_bounds__(PG_WAVE) void pgm_selinv_kernel(PgDev P, PgMarg Q)
{
    __shared__ double Wn[25 * 36];
    __shared__ double Lb[2][192];            // L[j + d][j], d = 0 .. 4, then 1 / diag(L[j][j])
    __shared__ double Gn[24 * 6];            // G_(j + d, j), d = 1 .. 4: row (d - 1) * 6 + i
    __shared__ double Mi[36];                // L_jj^-1
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, NB = P.NB;
    const auto fetch = [&](int b, int idx) {
        if (idx < 180) { const int d = idx / 36; return b + d < NB ? P.Lrow[(size_t(b + d) * PG_SLOTS + d) * 36 + idx % 36] : 0.0; }
        return P.Linv[size_t(b) * 6 + (idx - 180)];
    };
    for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) Lb[0][idx] = fetch(NB - 1, idx); }
    __syncthreads();
    for (int j = NB - 1; j >= 0; --j) {
        const int buf = (NB - 1 - j) & 1;
        double pre[3] = {0.0, 0.0, 0.0};
        if (j > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) pre[q] = fetch(j - 1, idx); }
        }
        const double *Lq = Lb[buf];
        if (t < 24) {                        // one row of G = L_(j + d, j) L_jj^-1: g L_jj = l, from the last column back
            const int d = 1 + t / 6, i = t % 6;
            double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (j + d < NB)
                for (int c = 5; c >= 0; --c) {
                    double v = Lq[d * 36 + i * 6 + c];
                    for (int q = c + 1; q < 6; ++q) v -= g[q] * Lq[q * 6 + c];
                    g[c] = v * Lq[180 + c];
                }
            for (int c = 0; c < 6; ++c) Gn[t * 6 + c] = g[c];
        } else if (t < 30) {                 // one column of L_jj^-1
            const int c = t - 24;
            double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            x[c] = Lq[180 + c];
            for (int r = c + 1; r < 6; ++r) {
                double v = 0.0;
                for (int q = c; q < r; ++q) v -= Lq[r * 6 + q] * x[q];
                x[r] = v * Lq[180 + r];
            }
            for (int r = 0; r < 6; ++r) Mi[r * 6 + c] = x[r];
        }
        __syncthreads();
        for (int idx = t; idx < 144; idx += PG_WAVE) {
            const int d = 1 + idx / 36, a = (idx % 36) / 6, c = idx % 6, i = j + d;
            if (i < NB) {
                double v = 0.0;
                for (int dk = 1; dk <= 4; ++dk) {
                    const int k = j + dk;
                    if (k < NB) {
                        const double *Sik = Wn + pgm_win_slot(i, k) * 36 + a * 6;
                        for (int q = 0; q < 6; ++q) v += Sik[q] * Gn[((dk - 1) * 6 + q) * 6 + c];
                    }
                }
                v = -v;
                Wn[pgm_win_slot(i, j) * 36 + a * 6 + c] = v;
                Wn[pgm_win_slot(j, i) * 36 + c * 6 + a] = v;
                Q.Sband[(size_t(j) * PG_SLOTS + d) * 36 + a * 6 + c] = v;
            }
        }
        __syncthreads();
        if (t < 36) {
            const int a = t / 6, c = t % 6;
            if (c <= a) {
                double v = 0.0;
                for (int q = a; q < 6; ++q) v += Mi[q * 6 + a] * Mi[q * 6 + c];
                for (int dk = 1; dk <= 4; ++dk) {
                    const int k = j + dk;
                    if (k < NB) {
                        const double *Sjk = Wn + pgm_win_slot(j, k) * 36 + a * 6;
                        for (int q = 0; q < 6; ++q) v -= Sjk[q] * Gn[((dk - 1) * 6 + q) * 6 + c];
                    }
                }
                Wn[pgm_win_slot(j, j) * 36 + a * 6 + c] = v;
                Wn[pgm_win_slot(j, j) * 36 + c * 6 + a] = v;
                Q.Sband[size_t(j) * PG_SLOTS * 36 + a * 6 + c] = v;
                Q.Sband[size_t(j) * PG_SLOTS * 36 + c * 6 + a] = v;
            }
        }
        if (j > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) Lb[buf ^ 1][idx] = pre[q]; }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(PG_WAVE) void pgm_zback_kernel(PgDev P)
{
    __shared__ double Lb[2][192];
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int t = threadIdx.x, col = blockIdx.x * PG_WAVE + t, NB = P.NB, ncp = P.ncp;
    if (P.m == 0) return;
    const bool active = col < P.m;
    const auto fetch = [&](int b, int idx) {
        if (idx < 180) { const int d = idx / 36; return b + d < NB ? P.Lrow[(size_t(b + d) * PG_SLOTS + d) * 36 + idx % 36] : 0.0; }
        return P.Linv[size_t(b) * 6 + (idx - 180)];
    };
    double zp[4][6];
    for (int d = 0; d < 4; ++d)
        for (int c = 0; c < 6; ++c) zp[d][c] = 0.0;
    for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) Lb[0][idx] = fetch(NB - 1, idx); }
    __syncthreads();
    for (int b = NB - 1; b >= 0; --b) {
        const int buf = (NB - 1 - b) & 1;
        double pre[3] = {0.0, 0.0, 0.0};
        if (b > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) pre[q] = fetch(b - 1, idx); }
        }
        const double *Lq = Lb[buf];
        double acc[6], z[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) acc[c] = active ? P.Y[(size_t(b) * 6 + c) * ncp + col] : 0.0;
#pragma unroll
        for (int d = 1; d <= 4; ++d)
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) acc[c] -= Lq[d * 36 + r * 6 + c] * zp[d - 1][r];
#pragma unroll
        for (int c = 5; c >= 0; --c) {
            double v = acc[c];
#pragma unroll
            for (int r = c + 1; r < 6; ++r) v -= Lq[r * 6 + c] * z[r];
            z[c] = v * Lq[180 + c];
        }
        if (active)
            for (int c = 0; c < 6; ++c) P.Y[(size_t(b) * 6 + c) * ncp + col] = z[c];
#pragma unroll
        for (int d = 3; d >= 1; --d)
#pragma unroll
            for (int c = 0; c < 6; ++c) zp[d][c] = zp[d - 1][c];
#pragma unroll
        for (int c = 0; c < 6; ++c) zp[0][c] = z[c];
        if (b > 0) {
#pragma unroll
            for (int q = 0; q < 3; ++q) { const int idx = t + q * PG_WAVE; if (idx < 186) Lb[buf ^ 1][idx] = pre[q]; }
        }
        __syncthreads();
    }
}

// workgroup: rows r0 .. r0 + 63 of the Y buffer (right-hand sides), every panel. v_mfma_f64_16x16x4_f64 as pg_gram_kernel documents it: A[row][k] = X[r0 + 16 w + row]
// [j0 + k] (a strided load: 16 rows, 4 consecutive doubles each), B[k][col] = U[j0 + k][k0 + 16 c + col] (16 consecutive doubles per quarter wavefront).
__global__ __launch_bounds__(PG_TPB) void pgm_trsm_kernel(PgDev P, PgMarg Q)
{
    __shared__ double Xl[PG_PANEL * (PG_PANEL + 1)];
    __shared__ double xs[2][PG_PANEL];
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int m = P.m, n = P.n, ncp = P.ncp, T = Q.mp / PG_PANEL;
    const int t = threadIdx.x, w = t >> 6, l = t & 63, lr = l >> 4, lc = l & 15;
    const int r0 = int(blockIdx.x) * PG_PANEL;
    const size_t ldu = size_t(Q.ldu);
    const int arow = r0 + 16 * w + lc;
    const bool arow_ok = arow < n;
    const double *xa = P.Y + size_t(arow_ok ? arow : 0) * ncp;
    const int r = l, q = w;                  // the solve's thread (r, q): right-hand side r0 + r, unknowns 4 u + q of the panel
    const bool srow_ok = r0 + r < n;
    double *xrow = P.Y + size_t(srow_ok ? r0 + r : 0) * ncp;
    for (int k = 0; k < T; ++k) {
        const int k0 = k * PG_PANEL;
        pg_d4 acc[4];
        for (int c = 0; c < 4; ++c) acc[c] = pg_d4{0.0, 0.0, 0.0, 0.0};
        for (int j0 = 0; j0 < k0; j0 += 16) {            // (k0 is a multiple of 64) four steps' operands in flight
            double av[4], bv[4][4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                av[u] = arow_ok ? xa[j0 + 4 * u + lr] : 0.0;
                const double *ub = Q.U + size_t(j0 + 4 * u + lr) * ldu + k0 + lc;
#pragma unroll
                for (int c = 0; c < 4; ++c) bv[u][c] = ub[16 * c];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[u], bv[u][c], acc[c], 0, 0, 0);
        }
        for (int c = 0; c < 4; ++c)
            for (int e = 0; e < 4; ++e) {
                const int rr = 16 * w + lr + 4 * e, cc = 16 * c + lc;
                const double x0 = (r0 + rr < n && k0 + cc < m) ? P.Y[size_t(r0 + rr) * ncp + k0 + cc] : 0.0;
                Xl[rr * (PG_PANEL + 1) + cc] = x0 - acc[c][e];
            }
        __syncthreads();
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = Xl[r * (PG_PANEL + 1) + 4 * u + q];
        const double *Uk = Q.U + size_t(k0) * ldu + k0;
#pragma unroll
        for (int c = 0; c < PG_PANEL; ++c) {
            if (q == (c & 3)) {
                const bool col_ok = k0 + c < m;
                const double x = col_ok ? v[c >> 2] / Uk[size_t(c) * ldu + c] : 0.0;
                xs[c & 1][r] = x;
                if (col_ok && srow_ok) xrow[k0 + c] = x;
            }
            __syncthreads();
            const double x = xs[c & 1][r];
#pragma unroll
            for (int u = c >> 2; u < 16; ++u)
                if (4 * u + q > c) v[u] -= Uk[size_t(c) * ldu + 4 * u + q] * x;
        }
        __syncthreads();                     // the panel's solved columns are read by the next panel's update, by other lanes of this workgroup
    }
}

__global__ __launch_bounds__(PG_WAVE) void pgm_tail_kernel(PgDev P, PgMarg Q)
{
    const PgState &S = *P.st;
    if (S.done || !S.lin_ok) return;
    const int k = int(blockIdx.x), t = threadIdx.x;
    double *lo = Q.out + size_t(k) * 36, *so = Q.out + (size_t(P.M) + k) * 36;
    if (k == 0) {                            // the gauge: block `first` is constant
        if (t < 36) { lo[t] = 0.0; so[t] = 0.0; }
        return;
    }
    const int b = k - 1;
    double g[21];
    for (int e = 0; e < 21; ++e) g[e] = 0.0;
    const double *X = P.Y + size_t(b) * 6 * P.ncp;
    for (int c = t; c < P.m; c += PG_WAVE) {
        double x[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) x[a] = X[size_t(a) * P.ncp + c];
        int e = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c2 = 0; c2 <= a; ++c2) g[e++] += x[a] * x[c2];
    }
    wave_sum(g);
    if (t != 0) return;
    double Sg[36], St[36];
    const double *Bi = Q.Sband + size_t(b) * PG_SLOTS * 36;
    int e = 0;
    for (int a = 0; a < 6; ++a)
        for (int c2 = 0; c2 <= a; ++c2) {
            const double v = Bi[a * 6 + c2] - g[e++];
            Sg[a * 6 + c2] = v; Sg[c2 * 6 + a] = v;
        }
    pgm_to_store(Sg, P.kf[P.first + k].pose, St);
    for (int c = 0; c < 36; ++c) { lo[c] = Sg[c]; so[c] = St[c]; }
}

// mlh_pg_marginals: the fixed launch list of pg_marg_host.hpp's pgm_launches, ONE host wait (the blocks and the state record land together)
int marginals_run(mlh_ctx *ctx, int cur_index, const mlh_pg_opts &o, int32_t form, double *covs, mlh_pg_marginals_result *res)
{
    const char *entry = "mlh_pg_marginals";
    PgStore &G = ctx->pg;
    { const int rc = pg_gate(ctx, entry); if (rc) return rc; }
    PgDev P;
    { const int rc = pg_problem(ctx, entry, cur_index, o, P); if (rc) return rc; }
    G.invalidate_marginals();                // no earlier result stays valid, whatever becomes of this call
    const size_t out_bytes = pgm_out_doubles(P.M) * sizeof(double), work_bytes = pgm_work_doubles(P.M, P.L) * sizeof(double), host_bytes = size_t(36) * P.M * sizeof(double);
    {
        const size_t before = G.marg_out.cap + G.marg_work.cap;
        MLH_HIP(ctx, G.marg_out.ensure(out_bytes));
        MLH_HIP(ctx, G.marg_work.ensure(work_bytes));
        if (G.marg_out.cap + G.marg_work.cap != before) ++G.allocations;
        MLH_HIP(ctx, G.h_marg.ensure(host_bytes, host_bytes / 4));
    }
    PgMarg Q;
    Q.Sband = G.marg_work.as<double>();
    Q.mp = int(pgm_panel_cols(P.L));
    if (P.L <= PG_MAX_LOOPS) { Q.U = Q.Sband + pgm_factor_offset(P.M); Q.ldu = Q.mp; }
    else { Q.U = P.C; Q.ldu = P.ld; }
    Q.out = G.marg_out.as<double>();
    hipStream_t st = ctx->stream;
    { const int rc = pg_enqueue_begin(ctx, P, 1, 1e4); if (rc) return rc; }
    if (P.NB > 0) {
        MLH_LAUNCH(pg_assemble_kernel, dim3(pg_blocks(size_t(P.NB) * PG_SLOTS)), dim3(PG_TPB), 0, st, P, 1);
        MLH_LAUNCH(pgm_unit_kernel, dim3(pg_blocks(P.n)), dim3(PG_TPB), 0, st, P);
        MLH_LAUNCH(pg_factor_kernel, dim3(1), dim3(PG_WAVE), 0, st, P, 0, 0);
        G.launches += 3;
        { const int rc = pg_enqueue_reduce(ctx, P, nullptr, 1); if (rc) return rc; }
        const int pack_blocks = P.T ? P.T : std::max(1, std::min(1024, pg_blocks(size_t(Q.mp) * Q.mp)));
        MLH_LAUNCH(pgm_pack_kernel, dim3(pack_blocks), dim3(PG_TPB), 0, st, P, Q);
        MLH_LAUNCH(pgm_selinv_kernel, dim3(1), dim3(PG_WAVE), 0, st, P, Q);
        MLH_LAUNCH(pgm_zback_kernel, dim3(std::max(1, (P.m + PG_WAVE - 1) / PG_WAVE)), dim3(PG_WAVE), 0, st, P);
        MLH_LAUNCH(pgm_trsm_kernel, dim3((P.n + PG_PANEL - 1) / PG_PANEL), dim3(PG_TPB), 0, st, P, Q);
        G.launches += 4;
    }
    MLH_LAUNCH(pgm_tail_kernel, dim3(P.M), dim3(PG_WAVE), 0, st, P, Q);
    ++G.launches;
    MLH_HIP(ctx, hipGetLastError());
    MLH_HIP(ctx, hipMemcpyAsync(G.h_marg.p, Q.out + (form == MLH_PG_COV_STORE ? size_t(36) * P.M : 0), host_bytes, hipMemcpyDeviceToHost, st));
    PgState S;
    { const int rc = pg_fetch_state(ctx, S); if (rc) return rc; }
    std::memset(res, 0, sizeof(*res));
    res->ok = S.lin_ok ? 1 : 0;
    res->n_keyframes = P.M; res->n_loops = P.L; res->first_index = P.first;
    res->launches = G.launches; res->host_waits = G.host_waits;
    if (res->ok) {
        if (covs) std::memcpy(covs, G.h_marg.p, host_bytes);
        G.marg_valid = true; G.marg_first = P.first; G.marg_cur = P.cur;
    }
    if (ctx->prof.mask) prof_collect(ctx);
    return MLH_OK;
}
