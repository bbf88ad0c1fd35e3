// radiance_grad.hip — rt_radiance_grad: the gradient of path-traced radiance with respect to the solid texture colours,
// the metal albedos and the background, along caller-given rays.  The kernels and their launcher (launch.h) in an object
// of their own, so that no kernel of another object moves.
//
// With a fixed seed no scatter direction depends on a colour and _ray_color has no Russian roulette, so a path's
// radiance is a product: the attenuations a_0 .. a_{k-1} of its k scatter vertices times what ended it (a light's
// emission or the background, E).  k_radiance_grad walks rt_radiance_rays' path (radiance_loop.inc's loop: the same
// trace_world, world_surface, cooperative sphere draw and scatter calls in the same order, the same claim by ballot
// rank), records a GradVertex per scatter, and at a path's end walks the records back (art.h states the products op for
// op).  Contributions are summed exactly: each f64 as a 192-bit integer (grad_fixed.h) with integer atomics, carries by
// hand, rounded once by k_grad_finish -- the gradient's bits depend on neither the grid nor the order of the rays.
// Every path adds to the background's row or a lamp's, and most paths to a few large surfaces' rows.  Two remedies, both
// exact because integer sums commute: the lanes of a wave whose paths end in the same loop iteration walk back together,
// and at each step the lanes that add to the same row sum their integers in LDS first (wave_add), one lane then adding
// the sum; and the accumulator table exists in up to kGradMaxCopies copies, a block adding to copy blockIdx.x % copies,
// which k_grad_finish sums.
#include <algorithm>

#include "art.h"
#include "path_work.h"
#include "ray_launch.h"
#include "grad_fixed.h"

namespace art {

// Waves per SIMD, as k_radiance_rays' HBM-scene forms: 168 VGPRs
constexpr int kGradWaves = 3;

// Dynamic LDS of a k_radiance_grad block: [traversal stacks: `stack` rows x kBlock lanes][jump table][job][a row of
// accumulator limbs per wave: wave_add's]
__host__ __device__ constexpr size_t grad_jump_offset(uint32_t stack) { return sizeof(int32_t) * stack * kBlock; }
__host__ __device__ constexpr size_t grad_scratch_offset(uint32_t stack) { return (grad_jump_offset(stack) + kJumpBytes + sizeof(GradJob) + 7u) & ~size_t(7); }
__host__ __device__ constexpr size_t grad_lds_bytes(uint32_t stack) {
    return grad_scratch_offset(stack) + sizeof(unsigned long long) * kGradRowLimbs * (kBlock / 64);
}

// tex_value (device.h) with the solid texture the value resolved to: `solid` is its index, or -1 for a noise or image
// value (and for the error colour).  The same doubles as tex_value.
template <uint32_t TF>
__device__ __forceinline__ V3 tex_value_id(const DevScene& S, int32_t ti, double u, double v, V3 p, int32_t& solid) {
    solid = -1;
    for (int level = 0; level < 4; ++level) {
        const TexRec& t = S.texs[ti];
        if (TF == TF_SOLID || t.type == TEX_SOLID) {
            solid = ti;
            return ld3(t.c);
        }
        if ((TF & TF_CHECKER) && t.type == TEX_CHECKER) {
            ti = checker_odd(p) ? t.odd : t.even;
            continue;
        }
        if ((TF & TF_NOISE) && t.type == TEX_NOISE) {
            const V3 q = t.scale * p;
            const double n = perlin_call(&S.perlins[t.perlin], q.x, q.y, q.z);
            const double h = (1.0 + n) * 0.5;
            return mk(h, h, h);
        }
        if ((TF & TF_IMAGE) && t.type == TEX_IMAGE) return image_value(S, t.image, u, v);
        if ((TF & (TF_IMAGE | TF_BARY)) && t.type == TEX_BARY_IMAGE) {
            const double w = 1.0 - u - v;
            return image_value(S, t.image, u * t.uv[0] + v * t.uv[2] + w * t.uv[4], u * t.uv[1] + v * t.uv[3] + w * t.uv[5]);
        }
        break;
    }
    return mk(0.0, 1.0, 1.0);
}
// mat_tex_value (device.h) likewise: the inlined copy of a MATF_SOLID record is its texture m.tex
template <uint32_t TF>
__device__ __forceinline__ V3 mat_tex_value_id(const DevScene& S, const MatRec& m, double u, double v, V3 p, int32_t& solid) {
    if (m.flags & MATF_SOLID) {
        solid = m.tex;
        return ld3(m.albedo);
    }
    return tex_value_id<TF>(S, m.tex, u, v, p, solid);
}

// limb[0..2] += f, exactly, with integer atomics (global memory or LDS): limb by limb, a limb's carry (read from the
// atomic's return) added to the next; a zero limb with no carry adds nothing.
__device__ __forceinline__ void grad_add_fix(unsigned long long* limb, const Fix192& f) {
    uint64_t carry = 0;
    if (f.w[0]) {
        const uint64_t old = atomicAdd(limb, static_cast<unsigned long long>(f.w[0]));
        carry = old + f.w[0] < old ? 1u : 0u;
    }
    const uint64_t a1 = f.w[1] + carry;
    carry = a1 < carry ? 1u : 0u;  // (then a1 is 0)
    if (a1) {
        const uint64_t old = atomicAdd(limb + 1, static_cast<unsigned long long>(a1));
        carry += old + a1 < old ? 1u : 0u;
    }
    const uint64_t a2 = f.w[2] + carry;
    if (a2) atomicAdd(limb + 2, static_cast<unsigned long long>(a2));
}
// row += c, exactly: each colour as a Fix192.  A contribution grad_fixed.h refuses sets the row's NaN flag.
__device__ __forceinline__ void grad_add(unsigned long long* row, V3 c) {
    const double v[3] = {c.x, c.y, c.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        Fix192 f;
        if (fix_from_double(v[a], f)) grad_add_fix(row + 3 * a, f);
        else atomicOr(row + 9, 1ull);
    }
}
// Every lane with `has` adds c to row `row` of the table acc.  The lanes of a row that several lanes add to sum in the
// wave's LDS row `scratch` (zero on entry and on return) with the same limb arithmetic, and the first of them adds that
// sum to the table: one set of global atomics per distinct row instead of one per lane.  A lane alone on its row adds
// by itself, after the loop and together with the other such lanes.  Called by the whole wave.
__device__ __forceinline__ void wave_add(unsigned long long* acc, unsigned long long* scratch, uint32_t lane, bool has, uint32_t row, V3 c) {
    uint64_t todo = __ballot(has);
    bool alone = false;
    while (todo) {
        const int leader = __ffsll(static_cast<unsigned long long>(todo)) - 1;
        const uint32_t r = static_cast<uint32_t>(__shfl(static_cast<int>(row), leader));
        const bool mine = has && row == r;
        const uint64_t members = __ballot(mine);
        if (__popcll(members) == 1) {
            alone = alone || mine;
        } else {
            if (mine) grad_add(scratch, c);
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup", "local");  // the wave's LDS atomics above, before the reads below
            if (lane == static_cast<uint32_t>(leader)) {
                unsigned long long* dst = acc + static_cast<size_t>(r) * kGradRowLimbs;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    Fix192 f;
                    f.w[0] = atomicExch(scratch + 3 * a, 0ull);
                    f.w[1] = atomicExch(scratch + 3 * a + 1, 0ull);
                    f.w[2] = atomicExch(scratch + 3 * a + 2, 0ull);
                    grad_add_fix(dst + 3 * a, f);
                }
                if (atomicExch(scratch + 9, 0ull)) atomicOr(dst + 9, 1ull);
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup", "local");
        }
        todo &= ~members;
    }
    if (alone) grad_add(acc + static_cast<size_t>(row) * kGradRowLimbs, c);
}

template <uint32_t F, uint32_t TF>
__global__ __launch_bounds__(kBlock, kGradWaves) void k_radiance_grad(DevScene S, GradJob job0) {
    constexpr int B = kBlock;
    constexpr bool L = false;
    extern __shared__ __align__(16) uint8_t smem[];
    StackT<L>* stk = reinterpret_cast<StackT<L>*>(smem) + B + stack_column<L>(threadIdx.x);
    stk[-B] = static_cast<StackT<L>>(kNodeEmpty);
    JumpEntry* jt = reinterpret_cast<JumpEntry*>(smem + grad_jump_offset(job0.path.stack));
    if (threadIdx.x < static_cast<uint32_t>(kJumpEntries)) jt[threadIdx.x] = pcg_jump(3u * threadIdx.x);
    // the job is read from LDS where a path starts or ends, as k_radiance_rays reads it
    const GradJob& gjob = *reinterpret_cast<const GradJob*>(jt + kJumpEntries);
    if (threadIdx.x == 0) *reinterpret_cast<GradJob*>(jt + kJumpEntries) = job0;
    unsigned long long* scratch = reinterpret_cast<unsigned long long*>(smem + grad_scratch_offset(job0.path.stack));
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
                int32_t solid = -1;
                if (mat.type == MAT_LIGHT || (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_ISOTROPIC)))
                    texc = mat_tex_value_id<TF>(S, mat, s.u, s.v, s.p, solid);
                if constexpr (kShared) {
                    if (scat && (mat.type == MAT_LAMBERTIAN || mat.type == MAT_METAL || mat.type == MAT_DIELECTRIC))
                        uv = unit(mat.type == MAT_LAMBERTIAN ? *pre : st.ray.d);
                }
                const V3* uvp = kShared ? &uv : nullptr;
                if (mat.type == MAT_LIGHT) {  // material.h:114-116; diffuse_light never scatters
                    st.L = st.L + st.T * texc;
                    ended = true, E = texc;
                    erow = solid >= 0 ? static_cast<uint32_t>(solid) : kGradNoRow;
                } else if (scat) {
                    V3 att, dir;
                    bool sc = false;
                    uint32_t row = kGradNoRow;
                    switch (mat.type) {
                        case MAT_LAMBERTIAN:
                            sc = scatter<MAT_LAMBERTIAN, TF>(S, mat, s, st, att, dir, pre, uvp, &texc);
                            if (solid >= 0) row = static_cast<uint32_t>(solid);
                            break;
                        case MAT_METAL:
                            sc = scatter<MAT_METAL, TF>(S, mat, s, st, att, dir, pre, uvp);
                            row = gjob.n_texs + static_cast<uint32_t>(s.mat);
                            break;
                        case MAT_DIELECTRIC: sc = scatter<MAT_DIELECTRIC, TF>(S, mat, s, st, att, dir, nullptr, uvp); break;
                        case MAT_ISOTROPIC:
                            sc = scatter<MAT_ISOTROPIC, TF>(S, mat, s, st, att, dir, pre, nullptr, &texc);
                            if (solid >= 0) row = static_cast<uint32_t>(solid);
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
            unsigned long long* acc = gjob.acc + static_cast<size_t>(blockIdx.x % gjob.copies) * gjob.rows * kGradRowLimbs;
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

// One thread per (row, column) of the three outputs: a colour column is the row's accumulator summed over the copies
// and rounded once (NaN when any copy's flag is set), every other column +0.0.
__global__ __launch_bounds__(256) void k_grad_finish(const unsigned long long* acc, uint32_t copies, uint32_t rows, uint32_t n_texs, uint32_t n_mats,
                                                     double* gt, double* gm, double* gb) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t nt = n_texs * RT_TEXTURE_DOUBLES, nm = n_mats * RT_MATERIAL_DOUBLES;
    if (e >= nt + nm + 3) return;
    uint32_t row, col;
    double* out;
    if (e < nt) row = e / RT_TEXTURE_DOUBLES, col = e % RT_TEXTURE_DOUBLES, out = gt ? gt + e : nullptr;
    else if (e < nt + nm) row = n_texs + (e - nt) / RT_MATERIAL_DOUBLES, col = (e - nt) % RT_MATERIAL_DOUBLES, out = gm ? gm + (e - nt) : nullptr;
    else row = rows - 1, col = e - nt - nm, out = gb ? gb + col : nullptr;
    if (!out) return;
    if (col >= 3) {
        *out = 0.0;
        return;
    }
    Fix192 sum{{0, 0, 0}};
    unsigned long long bad = 0;
    for (uint32_t c = 0; c < copies; ++c) {
        const unsigned long long* r = acc + (static_cast<size_t>(c) * rows + row) * kGradRowLimbs;
        const Fix192 part{{r[3 * col], r[3 * col + 1], r[3 * col + 2]}};
        fix_add(sum, part);
        bad |= r[9];
    }
    *out = bad ? fix_double(0x7ff8000000000000ull) : fix_to_double(sum);
}

// The kernel for this scene: every scene takes an HBM-scene form (with_ray_features' global_scene), the texture kinds
// as launch_radiance_job chooses them.  fn(kernel)
template <class Fn>
static void with_grad_kernel(const DeviceScene& ds, Fn&& fn) {
    with_ray_features(ds, true, [&](auto f, auto l) {
        constexpr uint32_t F = decltype(f)::value;
        if constexpr (!decltype(l)::value) {
            if (ds.tex_basic) return fn(&k_radiance_grad<F, kTexBasic>);
            if constexpr ((F & F_TRI) != 0)
                if (ds.tex_bary) return fn(&k_radiance_grad<F, kTexBary>);
            fn(&k_radiance_grad<F, TF_ALL>);
        }
    });
}

uint32_t radiance_grad_grid(const DeviceScene& ds, int num_cu, uint32_t P, uint32_t stack) {
    uint64_t full = 0;
    with_grad_kernel(ds, [&](auto kfn) {
        full = static_cast<uint64_t>(blocks_per_cu(reinterpret_cast<const void*>(kfn), kBlock, grad_lds_bytes(stack))) * static_cast<uint64_t>(num_cu);
    });
    const uint64_t need = (static_cast<uint64_t>(P) + kBlock - 1) / kBlock;
    return static_cast<uint32_t>(std::max<uint64_t>(1, std::min(full, need)));
}

void launch_radiance_grad(const DeviceScene& ds, hipStream_t st, const GradJob& job, uint32_t grid, uint32_t n, const double background[3],
                          uint32_t n_mats, double* grad_textures, double* grad_materials, double* grad_background) {
    DevScene S = ds.view;
    for (int a = 0; a < 3; ++a) S.bg[a] = background[a];
    with_grad_kernel(ds, [&](auto kfn) { hipLaunchKernelGGL(kfn, dim3(grid), dim3(kBlock), grad_lds_bytes(job.path.stack), st, S, job); });
    if (job.path.res) launch_radiance_sum(st, job.path.res, n, job.path.spp, job.path.radiance);
    const uint32_t cells = job.n_texs * RT_TEXTURE_DOUBLES + n_mats * RT_MATERIAL_DOUBLES + 3;
    if (grad_textures || grad_materials || grad_background)
        hipLaunchKernelGGL(k_grad_finish, dim3((cells + 255) / 256), dim3(256), 0, st, job.acc, job.copies, job.rows, job.n_texs, n_mats, grad_textures,
                           grad_materials, grad_background);
}

}  // namespace art
