// The body of the correspondence kernels of match.hip, included once per kernel: knn_features_kernel (W = TPB) and knn_features_wide_kernel (W = 512, 1024).
// One text, so that the argument batch, the prologue and the search are the same statements in both; included, not called, so that the 256-thread kernels
// compile to the code they had before the wide ones existed. In scope at the point of inclusion: P (the kernel's KParams) and the constants W, G, MB, K10, PRE,
// WARM, DEVM.
    __shared__ int s_run[(G == 16) ? (W / 16) * 2 * KNN_RUN_WORDS : (W / 8) * 2 * KNN_RUN_WORDS];
    __shared__ double s_pose[PRE ? 8 : 1];
    // every argument this launch's path reads -- tile counts, the prologue's, the search's of both kinds, ownership --: one batch, one wait
    const KindL k0 = P.k[0], k1 = P.k[1];
    {
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
        gn_prologue<PRE, MB, W>(P, pb, s_pose, f_ne, f_cnt2, f_scratch);
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
    if constexpr (G == 0) {
        if (K.lanes == 8) knn_features_body<8, MB, K10, PRE != 0, WARM, W>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat);
        else if (K.lanes == 32) knn_features_body<32, MB, K10, PRE != 0, WARM, W>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat);
        else knn_features_body<16, MB, K10, PRE != 0, WARM, W>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat);
    } else {
        knn_features_body<G, MB, K10, PRE != 0, WARM, W>(P, K, kind, own_mode, tile, s_run, s_pose, m_feat);
    }
