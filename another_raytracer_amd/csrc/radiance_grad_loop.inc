// radiance_grad_loop.inc — the persistent gradient path kernel, included once per kind of row:
//   GRAD_TEXELS 0  k_radiance_grad (radiance_grad.hip, GradJob): rows for solid textures, metals and the background
//   GRAD_TEXELS 1  k_texel_grad (texel_grad.hip, TexelJob): those, and a row per image texel in a second table
// One text, not one function template, for radiance_loop.inc's reason: included this way k_radiance_grad is the bytes
// it was when the text stood in radiance_grad.hip.  The texel form differs where a texture value is taken (the value
// comes with its row, grad_kernel.h's *_row functions, where the other form gets a solid texture's index) and in where
// a row's accumulator is (TexelRows); the loop, the records and the walk back are the same lines.
template <uint32_t F, uint32_t TF>
#if GRAD_TEXELS
__global__ __launch_bounds__(kBlock, kGradWaves) void k_texel_grad(DevScene S, TexelJob tjob0) {
    const GradJob& job0 = tjob0.g;
#else
__global__ __launch_bounds__(kBlock, kGradWaves) void k_radiance_grad(DevScene S, GradJob job0) {
#endif
    constexpr int B = kBlock;
    constexpr bool L = false;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + grad_jump_offset(job0.path.stack));
    if (threadIdx.x < static_cast<uint32_t>(kJumpEntries)) jt[threadIdx.x] = pcg_jump(3u * threadIdx.x);
    // the job is read from LDS where a path starts or ends, as k_radiance_rays reads it
#if GRAD_TEXELS
    const TexelJob& tjob = *reinterpret_cast<const TexelJob*>(jt + kJumpEntries);
    const GradJob& gjob = tjob.g;
    if (threadIdx.x == 0) *reinterpret_cast<TexelJob*>(jt + kJumpEntries) = tjob0;
    unsigned long long* scratch = reinterpret_cast<unsigned long long*>(smem + grad_scratch_offset(job0.path.stack, sizeof(TexelJob)));
#else
    const GradJob& gjob = *reinterpret_cast<const GradJob*>(jt + kJumpEntries);
    if (threadIdx.x == 0) *reinterpret_cast<GradJob*>(jt + kJumpEntries) = job0;
    unsigned long long* scratch = reinterpret_cast<unsigned long long*>(smem + grad_scratch_offset(job0.path.stack));
#endif
    if (threadIdx.x < kGradRowLimbs * (B / 64)) scratch[threadIdx.x] = 0;
    scratch += kGradRowLimbs * (threadIdx.x / 64);  // this wave's row
    __syncthreads();
    const RadianceJob& job = gjob.path;
    const uint8_t* lds = nullptr;
    const uint32_t lane = __lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const V3 bg = mk(S.bg[0], S.bg[1], S.bg[2]);
    const int max_depth = job0.path.max_depth;
    uint32_t cur = 0, end = 0;  // this wave's claimed path indices [cur, end): wave-uniform
    bool busy = false, drained = false;
    uint32_t q = 0;
    int depth = 0;
    PathState st;
    uint32_t segs = 0;
    for (;;) {
        const uint64_t idle = __ballot(!busy && !drained);
        if (idle) {
            const uint32_t n = static_cast<uint32_t>(__popcll(idle));
            const uint32_t rank = static_cast<uint32_t>(__popcll(idle & below));
            uint32_t p;
            if (cur + n > end) {
                uint32_t nb = 0;
                if (lane == 0) nb = atomicAdd(job.next, job.chunk);
                nb = __shfl(nb, 0);
                const uint32_t left = end - cur;
                p = rank < left ? cur + rank : nb + (rank - left);
                cur = nb + (n - left);
                end = nb + job.chunk;
            } else {
                p = cur + rank;
                cur += n;
            }
            if (!busy && !drained) {
                __asm__ volatile("" ::: "memory");  // keep the LDS job loads here
                if (p >= job.P) {
                    drained = true;
                } else {
                    const uint32_t i = job.fd_spp.div(p), s = p - i * job.spp;
                    const double* r = job.rays + 7 * static_cast<size_t>(i);
                    st.ray.o = mk(r[0], r[1], r[2]);
                    st.ray.d = mk(r[3], r[4], r[5]);
                    st.ray.tm = r[6];
                    st.rng = job.rng ? job.rng[p]
                                     : splitmix64(((static_cast<uint64_t>(job.id_base + i) << 32) | (job.sample_base + s)) ^ job.seed_mix);
                    st.T = mk(1.0, 1.0, 1.0);
                    q = p;
                    busy = true;
                    depth = 0;
                }
            }
        }
        if (__ballot(busy) == 0) {
            if (__ballot(!drained) == 0) break;
            continue;
        }
        double t;
        HitOut h{0, 0, kMatUnknown};
        bool hitw = false;
        Surf s;
        uint32_t mtype = MAT_LIGHT;
        if (busy) {
            ++segs;
            hitw = trace_world<F, B, L>(S, lds, st.ray, stk, st.rng, t, h);
            if (hitw) {
                world_surface<F, (TF & TF_IMAGE) != 0, (TF & (TF_IMAGE | TF_BARY)) != 0>(S, h, st.ray, t, s, uv_table(S));
                mtype = S.mats[s.mat].type;
            }
        }
        // the whole wave draws random_in_unit_sphere for its lambertian, metal and isotropic hits, as k_radiance_rays does
        const bool need = busy && hitw && (mtype == MAT_LAMBERTIAN || mtype == MAT_METAL || mtype == MAT_ISOTROPIC) && depth + 1 < max_depth;
        const V3 ps = coop_unit_sphere(need, st.rng, jt);
        const V3* pre = &ps;
        // what ended the lane's path in this iteration: its emission and the row that holds it (kGradNoRow with `ended`: a
        // noise or image light)
        bool ended = false;
        V3 E = mk(0.0, 0.0, 0.0);
        uint32_t erow = kGradNoRow;
        if (busy) {
            bool cont = false;
            st.L = mk(0.0, 0.0, 0.0);
            if (hitw) {
                const MatRec& mat = S.mats[s.mat];
                constexpr bool kShared = (TF & (TF_NOISE | TF_IMAGE)) != 0;
                const bool scat = depth + 1 < max_depth;
                // the texture value is always taken here, with the solid texture it resolved to; scatter gets it as texc
                V3 texc = mk(0.0, 0.0, 0.0), uv = mk(0.0, 0.0, 0.0);
#if GRAD_TEXELS
                uint32_t vrow = kGradNoRow;  // the value's row: a solid texture's, a texel's, or none
                if (mat.type == MAT_LIGHT || (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_ISOTROPIC)))
                    texc = mat_tex_value_row<TF>(S, tjob.image_row, mat, s.u, s.v, s.p, vrow);
#else
                int32_t solid = -1;
                if (mat.type == MAT_LIGHT || (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_ISOTROPIC)))
                    texc = mat_tex_value_id<TF>(S, mat, s.u, s.v, s.p, solid);
#endif
                if constexpr (kShared) {
                    if (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_METAL || mat.type == MAT_DIELECTRIC))
                        uv = unit(mat.type == MAT_LAMBERTIAN ? *pre : st.ray.d);
                }
                const V3* uvp = kShared ? &uv : nullptr;
                if (mat.type == MAT_LIGHT) {  // material.h:114-116; diffuse_light never scatters
                    st.L = st.L + st.T * texc;
                    ended = true, E = texc;
#if GRAD_TEXELS
                    erow = vrow;
#else
                    erow = solid >= 0 ? static_cast<uint32_t>(solid) : kGradNoRow;
#endif
                } else if (scat) {
                    V3 att, dir;
                    bool sc = false;
                    uint32_t row = kGradNoRow;
                    switch (mat.type) {
                        case MAT_LAMBERTIAN:
                            sc = scatter<MAT_LAMBERTIAN, TF>(S, mat, s, st, att, dir, pre, uvp, &texc);
#if GRAD_TEXELS
                            row = vrow;
#else
                            if (solid >= 0) row = static_cast<uint32_t>(solid);
#endif
                            break;
                        case MAT_METAL:
                            sc = scatter<MAT_METAL, TF>(S, mat, s, st, att, dir, pre, uvp);
                            row = gjob.n_texs + static_cast<uint32_t>(s.mat);
                            break;
                        case MAT_DIELECTRIC: sc = scatter<MAT_DIELECTRIC, TF>(S, mat, s, st, att, dir, nullptr, uvp); break;
                        case MAT_ISOTROPIC:
                            sc = scatter<MAT_ISOTROPIC, TF>(S, mat, s, st, att, dir, pre, nullptr, &texc);
#if GRAD_TEXELS
                            row = vrow;
#else
                            if (solid >= 0) row = static_cast<uint32_t>(solid);
#endif
                            break;
                        default: break;
                    }
                    if (sc && gjob.acc) {
                        // vertex `depth`: P_j = the throughput so far, a_j, the row
                        const size_t g = static_cast<size_t>(blockIdx.x) * B + threadIdx.x;
                        double2* rec = reinterpret_cast<double2*>(gjob.verts + (static_cast<size_t>(depth) * gjob.lanes + g));
                        rec[0] = make_double2(st.T.x, st.T.y);
                        rec[1] = make_double2(st.T.z, att.x);
                        rec[2] = make_double2(att.y, att.z);
                        reinterpret_cast<uint32_t*>(rec + 3)[0] = row;
                    }
                    if (sc) {
                        st.T = st.T * att;
                        st.ray.o = s.p;
                        st.ray.d = dir;
                        cont = true;
                    }
                }
            } else {  // engine.h:455-456: miss -> background
                st.L = st.L + st.T * bg;
                ended = true, E = bg;
                erow = gjob.rows - 1;
            }
            if (cont) {
                ++depth;
            } else {
                if (job.res) {
                    store_res<false>(job.res, q, st.L);
                } else if (job.radiance) {  // spp == 1: path q is ray q; the sum of one sample from +0.0
                    double* o = job.radiance + 3 * static_cast<size_t>(q);
                    o[0] = 0.0 + st.L.x;
                    o[1] = 0.0 + st.L.y;
                    o[2] = 0.0 + st.L.z;
                }
                busy = false;
            }
        }
        // The walk back (art.h), by the lanes whose path ended here, step by step together: the end adds w * P_k to the
        // row of E; then vertex j = k-1 .. 0 adds (w * P_j) * Q_j to its row, Q_{k-1} = E and Q_{j-1} = a_j * Q_j -- all
        // zero, and skipped, when E is zero.  (depth and st.T are the ended path's k and P_k until the lane starts anew.)
        if (gjob.acc && __ballot(ended)) {  // (acc null: no gradient asked for, nothing recorded, nothing to walk)
#if GRAD_TEXELS
            // the block's copy of each table: the counts differ (the texel table's is set by its byte budget)
            const TexelRows acc{gjob.acc + static_cast<size_t>(blockIdx.x % gjob.copies) * gjob.rows * kGradRowLimbs,
                                tjob.texel_acc + static_cast<size_t>(blockIdx.x % tjob.texel_copies) * tjob.n_texels * kGradRowLimbs, gjob.rows};
#else
            unsigned long long* acc = gjob.acc + static_cast<size_t>(blockIdx.x % gjob.copies) * gjob.rows * kGradRowLimbs;
#endif
            const size_t g = static_cast<size_t>(blockIdx.x) * B + threadIdx.x;
            V3 w = mk(0.0, 0.0, 0.0), Q = E, c = mk(0.0, 0.0, 0.0);
            uint32_t row = erow;
            int j = -1;
            if (ended) {
                const double* wp = gjob.weights + 3 * static_cast<size_t>(job.fd_spp.div(q));
                w = mk(wp[0], wp[1], wp[2]);
                c = w * st.T;
                if (E.x != 0.0 || E.y != 0.0 || E.z != 0.0) j = depth - 1;
            }
            bool step = ended;
            for (;;) {
                wave_add(acc, scratch, lane, step && row != kGradNoRow, row, c);
                step = step && j >= 0;
                if (__ballot(step) == 0) break;
                if (step) {
                    const double2* rec = reinterpret_cast<const double2*>(gjob.verts + (static_cast<size_t>(j) * gjob.lanes + g));
                    const double2 r0 = rec[0], r1 = rec[1], r2 = rec[2];
                    row = reinterpret_cast<const uint32_t*>(rec + 3)[0];
                    c = (w * mk(r0.x, r0.y, r1.x)) * Q;
                    Q = mk(r1.y, r2.x, r2.y) * Q;
                    --j;
                }
            }
        }
    }
    unsigned long long wsegs = segs;
    for (int off = 32; off > 0; off >>= 1) wsegs += __shfl_xor(wsegs, off);
    if (lane == 0) atomicAdd(job0.path.segments, wsegs);
}
