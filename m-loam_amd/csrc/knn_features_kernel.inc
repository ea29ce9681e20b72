// The body of the correspondence kernels of match.hip, included once per kernel: knn_features_kernel (W = TPB) and knn_features_wide_kernel (W = 512, 1024).
// One text, so that the argument batch, the prologue and the search are the same statements in both; included, not called, so that the 256-thread kernels
// compile to the code they had before the wide ones existed. In scope at the point of inclusion: P (the kernel's KParams) and the constants W, G, MB, K10, PRE,
// WARM, DEVM.
    __shared__ int s_run[(G == 16) ? (W / 16) * 2 * KNN_RUN_WORDS : (W / 8) * 2 * KNN_RUN_WORDS];
    __shared__ double s_pose[PRE ? 8 : 1];
    __shared__ float4 s_nbr[FIT ? ((G == 16) ? (W / 16) * 5 : (W / 8) * 5) : 1];      // FIT: the five winners of every query of the workgroup, for the lane that fits it
    // every argument this launch's path reads -- tile counts, the prologue's, the search's of both kinds, ownership --: one batch, one wait
    const KindL k0 = P.k[0], k1 = P.k[1];
    if constexpr (W != TPB) {
        // The wide kernels' batch. It also names the words that say how the prologue's records are laid out and, FIT, what the fit behind the search reads (the kind's
        // correspondence and covariance pointers, the gates, the loss, the rows' address): nothing is fetched again behind the search. A statement takes 30 operands:
        // a kind's four pointers go in as one vector, and so do rows_out / pre_rows; kb[0] is not read by a K = 5 kernel.
        const arg_i4 c0 = MLH_KIND_COUNTS(k0), c1 = MLH_KIND_COUNTS(k1), d0 = MLH_GRID_DIMS(k0), d1 = MLH_GRID_DIMS(k1), w = MLH_WORDS(P);
        const arg_f4 o0 = MLH_GRID_ORIGIN(k0), o1 = MLH_GRID_ORIGIN(k1);
        typedef unsigned long long u64_;
        const arg_u4 p0{u64_(k0.feat), u64_(k0.covd), u64_(k0.nbr), u64_(k0.corr)}, p1{u64_(k1.feat), u64_(k1.covd), u64_(k1.nbr), u64_(k1.corr)};
        const u64_ ro = u64_(P.rows_out);
        const arg_i4 fw{int(unsigned(ro)), int(unsigned(ro >> 32)), P.pre_rows, P.fit_pad_};
        const arg_f2 gate{P.min_match_sq_dis, P.min_plane_dis};
        const arg_d2 loss{P.huber_delta, P.cov_measurement_trace};
#define MLH_KNN_KINDS_WIDE "s"(p0), "s"(c0), "s"(k0.lanes), "s"(k0.grid.sorted), "s"(k0.grid.raw), "s"(k0.grid.cell_start), "s"(o0), "s"(d0), "s"(p1), "s"(c1), "s"(k1.lanes), \
                           "s"(k1.grid.sorted), "s"(k1.grid.raw), "s"(k1.grid.cell_start), "s"(o1), "s"(d1), "s"(w)
        if constexpr (PRE == 0) {
            const arg_d4 ip0{P.init_pose[0], P.init_pose[1], P.init_pose[2], P.init_pose[3]};
            const arg_d2 ip1{P.init_pose[4], P.init_pose[5]};
            const double ip2 = P.init_pose[6];
            const double *const pose_b0 = P.pose_b0, *const pose_bn = P.pose_bn;
            asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS_WIDE, "s"(ip0), "s"(ip1), "s"(ip2), "s"(pose_b0), "s"(pose_bn));
        } else {
            const double *const x_prev = P.x_prev;
            double *const x_next = P.x_next, *const partials = P.partials;
            const int pre_tiles = P.pre_tiles, pre_from_init = P.pre_from_init;
            if constexpr (PRE == 1) {
                const double thre0 = P.thre_b[0];
                const int freeze0 = P.freeze_b[0];
                if constexpr (FIT) asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS_WIDE, "s"(x_prev), "s"(x_next), "s"(partials), "s"(pre_tiles), "s"(pre_from_init), "s"(thre0), "s"(freeze0), "s"(fw), "s"(gate), "s"(loss));
                else asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS_WIDE, "s"(x_prev), "s"(x_next), "s"(partials), "s"(pre_tiles), "s"(pre_from_init), "s"(thre0), "s"(freeze0), "s"(fw));
            } else {
                SolverState *const state = P.state;
                HostPublish *const pre_publish = P.pre_publish;
                const unsigned long long pre_publish_seq = P.pre_publish_seq;
                const double pre_thre = P.pre_thre;
                const int pre_freeze = P.pre_freeze;
                if constexpr (FIT) asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS_WIDE, "s"(x_prev), "s"(x_next), "s"(partials), "s"(pre_tiles), "s"(pre_from_init), "s"(state), "s"(pre_publish),
                                                "s"(pre_publish_seq), "s"(pre_thre), "s"(pre_freeze), "s"(fw), "s"(gate), "s"(loss));
                else asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS_WIDE, "s"(x_prev), "s"(x_next), "s"(partials), "s"(pre_tiles), "s"(pre_from_init), "s"(state), "s"(pre_publish),
                                  "s"(pre_publish_seq), "s"(pre_thre), "s"(pre_freeze), "s"(fw));
            }
        }
#undef MLH_KNN_KINDS_WIDE
    } else {
        const arg_i4 c0 = MLH_KIND_COUNTS(k0), c1 = MLH_KIND_COUNTS(k1), d0 = MLH_GRID_DIMS(k0), d1 = MLH_GRID_DIMS(k1), w = MLH_WORDS(P);
        const arg_f4 o0 = MLH_GRID_ORIGIN(k0), o1 = MLH_GRID_ORIGIN(k1);
        const int kb0 = P.kb[0];
#define MLH_KNN_KINDS "s"(k0.feat), "s"(k0.nbr), "s"(c0), "s"(k0.lanes), "s"(k0.grid.sorted), "s"(k0.grid.raw), "s"(k0.grid.cell_start), "s"(o0), "s"(d0), "s"(k1.feat), "s"(k1.nbr), \
                      "s"(c1), "s"(k1.lanes), "s"(k1.grid.sorted), "s"(k1.grid.raw), "s"(k1.grid.cell_start), "s"(o1), "s"(d1), "s"(w), "s"(kb0)
        if constexpr (PRE == 0) {
            const arg_d4 ip0{P.init_pose[0], P.init_pose[1], P.init_pose[2], P.init_pose[3]};
            const arg_d2 ip1{P.init_pose[4], P.init_pose[5]};
            const double ip2 = P.init_pose[6];
            const double *const pose_b0 = P.pose_b0, *const pose_bn = P.pose_bn;
            asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS, "s"(ip0), "s"(ip1), "s"(ip2), "s"(pose_b0), "s"(pose_bn));
        } else {
            // (a start pose in the arguments is read per lane, by index: nothing to name)
            const double *const x_prev = P.x_prev;
            double *const x_next = P.x_next, *const partials = P.partials;
            const int pre_tiles = P.pre_tiles, pre_from_init = P.pre_from_init;
            if constexpr (PRE == 1) {
                const double thre0 = P.thre_b[0];
                const int freeze0 = P.freeze_b[0];
                asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS, "s"(x_prev), "s"(x_next), "s"(partials), "s"(pre_tiles), "s"(pre_from_init), "s"(thre0), "s"(freeze0));
            } else {
                SolverState *const state = P.state;
                HostPublish *const pre_publish = P.pre_publish;
                const unsigned long long pre_publish_seq = P.pre_publish_seq;
                const double pre_thre = P.pre_thre;
                const int pre_freeze = P.pre_freeze;
                asm volatile("; kernel arguments in registers" ::MLH_KNN_KINDS, "s"(x_prev), "s"(x_next), "s"(partials), "s"(pre_tiles), "s"(pre_from_init), "s"(state), "s"(pre_publish),
                             "s"(pre_publish_seq), "s"(pre_thre), "s"(pre_freeze));
            }
        }
#undef MLH_KNN_KINDS
    }
    int m0 = k0.m, m1 = k1.m, ta0 = k0.tiles_a;
    int total = k0.tiles_a + k1.tiles_a;
    if constexpr (DEVM) {
        static_assert(G == 0 && !MB && PRE == 0, "device-side counts: per-kind lanes, one block, no prologue");
        m0 = P.m_dev[0]; m1 = P.m_dev[1];
        const int f0 = W / k0.lanes, f1 = W / k1.lanes;
        ta0 = (m0 + f0 - 1) / f0;
        total = ta0 + (m1 + f1 - 1) / f1;
        if ((int(blockIdx.x) >> 3) >= ((total + 7) >> 3)) return;     // (xcd_tile is a bijection only on the first 8 * ceil(total / 8) workgroups)
    }
    int tile = xcd_tile(total);
    if (tile >= total) return;
    const int kind = tile >= ta0 ? 1 : 0;
    // this workgroup's kind and the ownership word, as values the compiler cannot fetch again: behind the prologue it would rather re-read both kinds' arguments
    // and select once more than keep the selection in registers
    KindL K = pick_kind(kind != 0, k0, k1);
    int own_mode = P.own_mode;
    if constexpr (PRE != 0 && !MB) {
        asm volatile("" : "+s"(K.feat), "+s"(K.nbr), "+s"(K.nbr_stride), "+s"(K.lanes), "+s"(K.grid.sorted), "+s"(K.grid.raw), "+s"(K.grid.cell_start), "+s"(own_mode));
        // (the grid's origin and dimensions are left out: the compiler selects those four-word groups as vectors, on the vector unit)
    }
    // FIT: what the fit behind the search reads, held the same way
    [[maybe_unused]] uint32_t fit_flags = P.flags;
    [[maybe_unused]] float min_match_sq_dis = P.min_match_sq_dis, min_plane_dis = P.min_plane_dis;
    [[maybe_unused]] double huber_delta = P.huber_delta, cov_measurement_trace = P.cov_measurement_trace;
    [[maybe_unused]] double *rows_out = P.rows_out;
    [[maybe_unused]] int rows_before = 0, rows_made = 0, rows_all = 0;      // of the workgroup's kind: rows of the kinds in front, rows its wide tiles produce, rows its 256-feature tiles hold
    if constexpr (FIT) {
        const int qpw = W / ((G == 0) ? K.lanes : G) / 64;                   // wavefront rows per workgroup: 1 or 2
        rows_before = kind ? 4 * k0.tiles_b : 0;
        rows_made = K.tiles_a * qpw;
        rows_all = 4 * K.tiles_b;
        asm volatile("" : "+s"(K.corr), "+s"(K.covd), "+s"(fit_flags), "+s"(min_match_sq_dis), "+s"(min_plane_dis), "+s"(huber_delta), "+s"(cov_measurement_trace), "+s"(rows_out),
                     "+s"(rows_before), "+s"(rows_made), "+s"(rows_all));
    }
    if constexpr (PRE != 0) {
        __shared__ double f_ne[NE_STRIDE], f_cnt2[2], f_scratch[(GN_SUM_THREADS / 32) * 32];
        int pb = 0;
        bool writer = tile == 0;
        if constexpr (MB) {
            // pose blocks start on 256-slot boundaries and a workgroup serves 16 or 32 consecutive slots of ONE kind: all of them in one block. The block's pose is
            // written by the workgroup of its first surf tile (the host defers a solve over blocks only when every block has surf features)
            const int tk = kind ? tile - ta0 : tile;
            const int lanes = (G == 0) ? K.lanes : G;
            const int f0 = tk * (W / lanes);
            pb = block_of_slot(P.k[kind], P.n_blocks, f0);
            writer = kind == 0 && f0 == P.k[0].blk_start[pb];
        }
        MLH_KSTAGE(6);
        gn_prologue<PRE, MB, W, W != TPB>(P, pb, s_pose, f_ne, f_cnt2, f_scratch);      // (wide: the records may be a fused launch's rows)
        MLH_KSTAGE(7);
        if constexpr (PRE == 2) {
            __shared__ double s_chain[8];
            if (threadIdx.x == 0) {
                if (tile == 0) publish_final_pose(P, s_pose);
                double xc[7], out[7];
                for (int i = 0; i < 7; ++i) xc[i] = s_pose[i];
                double cp[7], cc[7];
                for (int i = 0; i < 7; ++i) { cp[i] = P.chain_prev[i]; cc[i] = P.chain_cur[i]; }
                chain_start_pose(xc, cp, cc, out);
                for (int i = 0; i < 7; ++i) s_chain[i] = out[i];
            }
            __syncthreads();
            if (threadIdx.x < 7) s_pose[threadIdx.x] = s_chain[threadIdx.x];
            __syncthreads();
        }
        if (writer && threadIdx.x < 7) P.x_next[7 * pb + threadIdx.x] = s_pose[threadIdx.x];
    }
    if (kind) tile -= ta0;
    const int m_feat = kind ? m1 : m0;
    // FIT: lane i of the workgroup's first wavefronts fits the workgroup's query i. Its feature (and covariance diagonal) is requested here, with the search's own
    // first loads, and waits in registers
    [[maybe_unused]] int fit_f = 0;
    [[maybe_unused]] float4 fit_fp = make_float4(0.f, 0.f, 0.f, -1.f), fit_cd = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (FIT) {
        const int fpb = W / ((G == 0) ? K.lanes : G);
        fit_f = tile * fpb + int(threadIdx.x);
        if (int(threadIdx.x) < fpb && fit_f < m_feat) {
            fit_fp = K.feat[fit_f];
            if ((fit_flags & MLH_FLAG_WITH_UA) && K.covd) fit_cd = K.covd[fit_f];
        }
    }
    if constexpr (G == 0) {
        if (K.lanes == 8) knn_features_body<8, MB, K10, PRE != 0, WARM, W, FIT>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat, s_nbr);
        else if (!FIT && K.lanes == 32) knn_features_body<32, MB, K10, PRE != 0, WARM, W>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat);     // (32 lanes: 32 queries per workgroup, never fused)
        else knn_features_body<16, MB, K10, PRE != 0, WARM, W, FIT>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat, s_nbr);
    } else {
        knn_features_body<G, MB, K10, PRE != 0, WARM, W, FIT>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat, s_nbr);
    }
    if constexpr (FIT) {
        const int fpb = W / ((G == 0) ? K.lanes : G);
        MLH_STAGE(blockIdx.x, 0);                               // (debug build only: the fused tail's stamps, by workgroup -- scripts/stageclock_knn.py reads the search's)
        __syncthreads();                                        // the winners are in s_nbr
        MLH_STAGE(blockIdx.x, 1);
        const int wave = int(threadIdx.x) >> 6;
        // the rows of the kind's last 256-feature tile that no workgroup produces: zeros, from a wavefront that does not fit
        if (tile == K.tiles_a - 1 && wave == W / 64 - 1) {
            for (int i = int(threadIdx.x) & 63; i < (rows_all - rows_made) * NE_STRIDE; i += 64) rows_out[size_t(rows_before + rows_made) * NE_STRIDE + i] = 0.0;
        }
        if (int(threadIdx.x) >= fpb) return;
        const q4 q{s_pose[3], s_pose[4], s_pose[5], s_pose[6]};
        const d3 t{s_pose[0], s_pose[1], s_pose[2]};
        bool valid = false;
        float coef[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (fit_f < m_feat) {
            float4 nbv[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) nbv[j] = s_nbr[int(threadIdx.x) * 5 + j];
            if (fit_fp.w >= 0.f) {
                valid = fit_feature<5, 5>(min_match_sq_dis, min_plane_dis, kind, nbv, coef);
                if (valid && (fit_flags & MLH_FLAG_CHECK_FOV)) {
                    float sx, sy, sz;
                    associate_to_map(q, t, fit_fp, sx, sy, sz);
                    valid = in_laser_fov(q, t, sx, sy, sz);
                }
            }
            Corr c;
#pragma unroll
            for (int i = 0; i < 6; ++i) c.c[i] = valid ? coef[i] : 0.f;
            c.valid = valid ? 1 : 0;
            c.pad = 0;
            K.corr[fit_f] = c;
        }
        MLH_STAGE(blockIdx.x, 2);
        const Lin L = eval_factor(valid, kind, d3{double(fit_fp.x), double(fit_fp.y), double(fit_fp.z)}, coef, valid ? feature_weight_pref(fit_flags, cov_measurement_trace, K, fit_cd) : 0.0, q, t);
        reduce_rows_wave(valid, L, huber_delta, (fit_flags & MLH_FLAG_NO_LOSS) != 0, kind, rows_out + size_t(rows_before + tile * (fpb / 64) + wave) * NE_STRIDE);
        MLH_STAGE(blockIdx.x, 3);
    }
