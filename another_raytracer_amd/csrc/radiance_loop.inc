// radiance_loop.inc — the persistent path kernel of radiance_rays.hip, which includes this text once per path source:
//   RADIANCE_KERNEL   the kernel's name, RADIANCE_JOB its job type (launch.h)
//   RADIANCE_CAMERAS  0: a path starts at a caller-given ray read from memory (k_radiance_rays, RadianceJob)
//                     1: at the camera ray of a view of the job's table (k_radiance_views, ViewsJob)
// One text, not one function template: a device function shared by two kernels is simplified on its own before it is
// inlined, and k_radiance_rays then comes out as other code (the same results, 4-8 bytes shorter or longer).  Included
// this way, the memory-source kernels are the bytes they were before the second source existed.
template <uint32_t F, bool L, uint32_t TF>
__global__ __launch_bounds__(L ? kBlockL : kBlock, L ? 1 : kRadianceWaves) void RADIANCE_KERNEL(DevScene S, RADIANCE_JOB job0) {
    constexpr int B = L ? kBlockL : kBlock;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem + (L ? kLdsImageBytes : 0u)) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + radiance_jump_offset(L, job0.stack));
    if (threadIdx.x < static_cast<uint32_t>(kJumpEntries)) jt[threadIdx.x] = pcg_jump(3u * threadIdx.x);
    // the job is read from LDS where a path starts or ends, as k_paths_g reads its pass geometry: held in SGPRs for the
    // whole loop beside the scene view, the kernel arguments spill into VGPR lanes
    const RADIANCE_JOB& job = *reinterpret_cast<const RADIANCE_JOB*>(jt + kJumpEntries);
    if (threadIdx.x == 0) *reinterpret_cast<RADIANCE_JOB*>(jt + kJumpEntries) = job0;
    if constexpr (L) load_lds_image<B>(S.lds_image, smem);
    __syncthreads();
    const uint8_t* lds = L ? smem : nullptr;
    const uint32_t lane = __lane_id();
    const uint64_t below = (1ull << lane) - 1ull;
    const V3 bg = mk(S.bg[0], S.bg[1], S.bg[2]);
    const int max_depth = job0.max_depth;
    uint32_t cur = 0, end = 0;  // this wave's claimed path indices [cur, end): wave-uniform
    bool busy = false, drained = false;
    uint32_t q = 0;
    int depth = 0;
    PathState st;
    uint32_t segs = 0;  // this lane's segments (32 bits: a register less in the loop; summed in 64)
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
#if RADIANCE_CAMERAS
                    // i = v * npix + ly * W + lx: the view's camera and seed from the table, the ray in registers
                    const uint32_t v = job.fd_npix.div(i), pixel = i - v * job.npix;
                    const uint32_t ly = job.fd_w.div(pixel), lx = pixel - ly * static_cast<uint32_t>(job.W);
                    view_cam_ray(job, job.views[v], s, static_cast<int>(lx), static_cast<int>(ly), st.ray, st.rng);
#else
                    const double* r = job.rays + 7 * static_cast<size_t>(i);
                    st.ray.o = mk(r[0], r[1], r[2]);
                    st.ray.d = mk(r[3], r[4], r[5]);
                    st.ray.tm = r[6];
                    st.rng = job.rng ? job.rng[p]
                                     : splitmix64(((static_cast<uint64_t>(job.id_base + i) << 32) | (job.sample_base + s)) ^ job.seed_mix);
#endif
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
        // the whole wave draws random_in_unit_sphere for its lambertian, metal and isotropic hits, as k_paths_g does
        const bool need = busy && hitw && (mtype == MAT_LAMBERTIAN || mtype == MAT_METAL || mtype == MAT_ISOTROPIC) && depth + 1 < max_depth;
        const V3 ps = coop_unit_sphere(need, st.rng, jt);
        const V3* pre = &ps;
        if (busy) {
            bool cont = false;
            // a live path's radiance is zero: only a miss or a light adds to it, and both end the path
            st.L = mk(0.0, 0.0, 0.0);
            if (hitw) {
                const MatRec& mat = S.mats[s.mat];
                // the steps several materials share, once for the wave (k_paths_g.h: kernels with noise or image textures)
                constexpr bool kShared = (TF & (TF_NOISE | TF_IMAGE)) != 0;
                V3 texc = mk(0.0, 0.0, 0.0), uv = mk(0.0, 0.0, 0.0);
                if constexpr (kShared) {
                    const bool scat = depth + 1 < max_depth;
                    if (mat.type == MAT_LIGHT || (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_ISOTROPIC)))
                        texc = mat_tex_value<TF>(S, mat, s.u, s.v, s.p);
                    if (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_METAL || mat.type == MAT_DIELECTRIC))
                        uv = unit(mat.type == MAT_LAMBERTIAN ? *pre : st.ray.d);
                }
                const V3* texp = kShared ? &texc : nullptr;
                const V3* uvp = kShared ? &uv : nullptr;
                if (mat.type == MAT_LIGHT) {  // material.h:114-116; diffuse_light never scatters
                    st.L = st.L + st.T * (texp ? *texp : mat_tex_value<TF>(S, mat, s.u, s.v, s.p));
                } else if (depth + 1 < max_depth) {
                    V3 att, dir;
                    bool sc = false;
                    switch (mat.type) {
                        case MAT_LAMBERTIAN: sc = scatter<MAT_LAMBERTIAN, TF>(S, mat, s, st, att, dir, pre, uvp, texp); break;
                        case MAT_METAL: sc = scatter<MAT_METAL, TF>(S, mat, s, st, att, dir, pre, uvp); break;
                        case MAT_DIELECTRIC: sc = scatter<MAT_DIELECTRIC, TF>(S, mat, s, st, att, dir, nullptr, uvp); break;
                        case MAT_ISOTROPIC: sc = scatter<MAT_ISOTROPIC, TF>(S, mat, s, st, att, dir, pre, nullptr, texp); break;
                        default: break;
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
            }
            if (cont) {
                ++depth;
            } else {
                if (job.res) {
                    store_res<false>(job.res, q, st.L);
                } else {  // spp == 1: path q is ray (pixel) q; the sum of one sample from +0.0
                    double* o = job.radiance + 3 * static_cast<size_t>(q);
                    o[0] = 0.0 + st.L.x;
                    o[1] = 0.0 + st.L.y;
                    o[2] = 0.0 + st.L.z;
                }
                busy = false;
            }
        }
    }
    unsigned long long wsegs = segs;
    for (int off = 32; off > 0; off >>= 1) wsegs += __shfl_xor(wsegs, off);
    if (lane == 0) atomicAdd(job0.segments, wsegs);
}
