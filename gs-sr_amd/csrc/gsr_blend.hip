// gsr_blend.hip -- per-tile alpha blend forward for the EWA / PLANE / SURFEL variants, and the launchers of both blend stages (the backward kernel
// is the splat-parallel one of gsr_blend_sp.hip).
//
// CDNA4 design (not the reference's 16x16-thread / shared-memory-batch / __syncthreads scheme):
//   * one 64-lane wavefront owns an 8x8 pixel sub-tile (4 waves = one 16x16 tile, same tile list, NO barriers,
//     each wave terminates on its own as soon as its 64 pixels are saturated);
//   * the tile's depth-sorted splat list is consumed 64 at a time: lane l fetches instance l's conservative
//     screen box, tests it against the wave's sub-tile, and a 64-bit ballot gives the queue of splats that can
//     touch this sub-tile at all -- non-contributing (pixel, splat) pairs are skipped a whole wave at a time;
//   * forward: the surviving candidates' packed records are staged in wave-private LDS by the lanes that tested them and read back
//     through a wave-uniform address (broadcast ds_read_b128), so the blend maths has VGPR operands only.
// Behaviour follows 3DGS forward.cu:261-374, PLANE forward.cu:273-407, SURFEL forward.cu:256-448 (thresholds, ordering, recurrences); see DESIGN.md.
#include "gsr_blend_common.h"
#include <algorithm>
#include "gsr_tile_sort.h"

// =================================================================================================== forward
// The pair loop's counter: one iteration fewer to go, none once no pixel of the wave blends any more (the early exit).  Two scalar instructions; as
// `live ? left - 1 : 0` the compiler folds the exit into the loop condition as 64-bit selects, eleven scalar instructions an iteration.
__device__ __forceinline__ uint32_t fwd_next_left(uint32_t left, uint64_t live)
{
    uint32_t r;
    asm("s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, %2, 0" : "=s"(r) : "s"(live), "s"(__builtin_amdgcn_readfirstlane((int)(left - 1u))) : "scc");
    return r;
}

template <int V>
__global__ void __launch_bounds__(256) k_blend_fwd(BlendParams p)
{
    constexpr int ST = (V == GSR_EWA) ? GSR_REC_EWA : (V == GSR_PLANE ? GSR_REC_PLANE : GSR_REC_SURFEL);
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    // [wave][record quarter][candidate slot]: private to the wave, no barrier.  20 KB for every variant (SURFEL needs them; eight workgroups per CU --
    // the wave limit -- fit either way): the sort prologue borrows the buffer and takes lists of up to 2048 entries in LDS instead of sending EWA's
    // beyond 1024 to the global-memory radix path (EWA at P = 1.5 M: 624 -> 663 it/s; neutral at 300k: blend forward 0.2207 vs 0.2204 ms)
    __shared__ float4 s_rec[(4 * ST * 64 > 1280) ? 4 * ST * 64 : 1280];
    const int tile = tile_of_block(blockIdx.x, p.gx * p.gy, p.tile_order, p.static_map);
    const int tx = tile % p.gx, ty = tile / p.gx;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int ox = tx * GSR_TILE + (wave & 1) * GSR_SUB, oy = ty * GSR_TILE + (wave >> 1) * GSR_SUB;
    const uint2 range = p.ranges[tile];
    if (p.depth_key) {
        // per-tile depth order, fused: the four waves put the tile's list in (depth, id) order before any of them blends (the only barriers of
        // the kernel; s_rec is free until the first batch is staged).  The backward reads the same list afterwards.
        TdsScratch sc; sc.tile_keys = p.tile_keys; sc.keys = p.scratch_keys; sc.ids = p.scratch_ids;
        tds_sort_tile_wg<(int)sizeof(s_rec)>(s_rec, p.list_rw + range.x, range.y > range.x ? range.y - range.x : 0u, range.x, (uint32_t)tile, p.depth_key, sc, p.sort_buckets != 0, p.list_any_order != 0);
    }
    if (p.status && blockIdx.x == 0 && threadIdx.x == 0) { const uint32_t R = *p.status_total; p.status[0] = R; if (R > p.status_cap) p.status[1] = 1u; }
    if (p.long_word && threadIdx.x == 0 && range.y > range.x && range.y - range.x > p.long_len) *p.long_word = range.y - range.x;      // feedback for the launch order
    if (ox >= p.W || oy >= p.H) return;                 // wave-uniform: this sub-tile is outside the image
    const int px = ox + (lane & 7), py = oy + (lane >> 3);
    const bool inside = px < p.W && py < p.H;
    const float pxf = (float)px, pyf = (float)py;
    const float fdx = (float)(lane & 7), fdy = (float)(lane >> 3);      // SURFEL: pixel offset inside the sub-tile
    const size_t HW = (size_t)p.W * p.H;
    const uint32_t pix_id = (uint32_t)p.W * py + px;

    float T = 1.0f;
    uint32_t last_contributor = 0;
    float C0 = 0, C1 = 0, C2 = 0;
    // Which pixels still blend, and every gate of the pair loop, are kept as 64-bit wave masks in SCALAR registers: the compares write them directly
    // (v_cmp -> SGPR pair, __builtin_amdgcn_fcmpf), they are combined on the scalar unit, and the lanes that apply the splat are selected through
    // inverse_ballot.  With `done` as a loop-carried bool the early-exit test __ballot(!done) cost a v_cndmask + v_cmp per pair on top of the
    // scalar bookkeeping of the bool's phi.  Predicates (LLVM fcmp numbering): 2 ogt, 4 olt, 5 ole, 11 uge, 13 ule, 14 une -- the unordered
    // forms reproduce the reference's negated tests (`!(a < b)` is true for NaN).
    uint64_t live = __ballot(inside);
    // SURFEL
    float N0 = 0, N1 = 0, N2 = 0, Dd = 0, M1 = 0, M2 = 0, distortion = 0, median_depth = 0;
    uint32_t median_contributor = 0; int surf_idx = -1;
    float mn0 = 0, mn1 = 0, mn2 = 0;
    // PLANE
    float A0 = 0, A1 = 0, A2 = 0, A3 = 0, A4 = 0;

    for (uint32_t base = range.x; base < range.y; base += GSR_WAVE) {
        if (live == 0) break;
        const uint32_t i = base + lane;
        const bool v = i < range.y;
        const uint32_t id = v ? p.point_list[i] : 0u;
        const bool hit = v && cull_hit<V>(p.cull, id, (float)ox, (float)oy);
        uint64_t m = __ballot(hit);
        // the ballot is what the splat-parallel backward needs to know about this (batch, quadrant): keep it (8 bytes per 64 entries)
        if (p.qmask && lane == 0) p.qmask[(((size_t)(range.x >> 6) + (size_t)tile + ((base - range.x) >> 6)) << 2) + wave] = m;
        // Every lane whose candidate survives the cull stages that candidate's packed record in the wave's LDS slots: one burst of vector
        // loads per 64 candidates instead of a scalar-load round trip per pair.  The pair loop reads the record back through a wave-uniform
        // LDS address (broadcast ds_read_b128), so the blend maths runs on VGPR operands only -- on gfx950 a VALU instruction with an SGPR
        // operand issues in ~4.2 cycles against ~2.7 for VGPR-only fma / mul / add (tools/microbench/valu_rate.hip), and the 6 v_mov the
        // two-SGPR fmas of the surfel intersection needed are gone.  Measured: surfel 0.234 -> 0.201 ms, EWA 0.233 -> 0.189, PLANE 0.199 -> 0.176.
#ifndef FWD_DIAG_NO_STAGE
        if (hit) {
#else
        if (hit && p.W < 0) {
#endif
            const float4* __restrict__ rr = p.rec + (size_t)id * ST;
            if constexpr (V == GSR_SURFEL) {
                // SURFEL: the staging lane also does the per-(splat, sub-tile) part of the ray-splat intersection.  p = k x l (k = px Tw - Tu, l = py Tw - Tv,
                // SURFEL forward.cu:351-357) is affine in the pixel: with (ox, oy) the sub-tile's first pixel, k0 = ox Tw - Tu, l0 = oy Tw - Tv,
                //     p(ox + dx, oy + dy) = k0 x l0 + dx (Tw x l0) + dy (k0 x Tw),
                // and the depth s . Tw.xy + Tw.z equals det[Tu Tv Tw] / p.z (record word D, gsr_preprocess.hip).  Staged: {P0, Px, Py, D, Tw.z, opacity,
                // centre - origin, normal, rgb} = 20 floats, so that a pixel pays 6 FMAs + 1 multiply for p and the depth instead of 15 instructions.
                const float4 r0 = rr[0], r1 = rr[1], r2 = rr[2], r3 = rr[3], r4 = rr[4];
                const float fox = (float)ox, foy = (float)oy;
                const float Tw0 = r1.z, Tw1 = r1.w, Tw2 = r2.x;
                const float kx = fox * Tw0 - r0.x, ky = fox * Tw1 - r0.y, kz = fox * Tw2 - r0.z;
                const float lx = foy * Tw0 - r0.w, ly = foy * Tw1 - r1.x, lz = foy * Tw2 - r1.y;
                float4* dst = s_rec + wave * ST * 64 + lane;
                dst[0 * 64] = make_float4(ky * lz - kz * ly, kz * lx - kx * lz, kx * ly - ky * lx, Tw1 * lz - Tw2 * ly);
                dst[1 * 64] = make_float4(Tw2 * lx - Tw0 * lz, Tw0 * ly - Tw1 * lx, ky * Tw2 - kz * Tw1, kz * Tw0 - kx * Tw2);
                dst[2 * 64] = make_float4(kx * Tw1 - ky * Tw0, r4.z, Tw2, r2.w);
                dst[3 * 64] = make_float4(r2.y - fox, r2.z - foy, r3.x, r3.y);
                dst[4 * 64] = make_float4(r3.z, r3.w, r4.x, r4.y);
            } else {
                // (staging the conic times log2(e), so that a pair pays exp2 instead of a multiply and a v_exp_f32: PLANE 0.1705 -> 0.168 ms, EWA 0.1695 -> 0.171, and
                // the three separately rounded products break the cancellation inside `power` of x20 needle splats -- test_needle_splats_are_not_culled_away;
                // removed, EXPERIMENTS.md (74))
#pragma unroll
                for (int k = 0; k < ST; k++) s_rec[(wave * ST + k) * 64 + lane] = rr[k];      // [wave][k][slot]: lane-contiguous 16-byte stores
            }
        }
#ifdef FWD_DIAG_NO_PAIRS      // diagnostic build only: the kernel without its pair loop (results are then wrong)
        m = 0;
#endif
#ifdef FWD_DIAG_NO_STAGE
        m = 0; if (lane == 99) s_rec[0] = make_float4(0.f, 0.f, 0.f, 0.f);
#endif
        // The slot a lane last blended, and the last one it blended at T > 0.5, are all the pair loop keeps of "which splat": the positions in the list and,
        // for the median, the normal and the gaussian's id are looked up once per batch below, while the batch is still staged.
        uint32_t slot_last = NONE, slot_med = NONE;
        for (uint32_t left = (uint32_t)__popcll(m); left != 0u; left = fwd_next_left(left, live)) {
            // the queue's next slot, and its removal: one scalar instruction each (as `m &= m - 1` the removal is three)
            uint32_t sl;
            asm("s_ff1_i32_b64 %0, %1" : "=s"(sl) : "s"(m));
            asm("s_bitset0_b64 %0, %1" : "+s"(m) : "s"(sl));
            const float4* lr = s_rec + wave * ST * 64 + sl;
#define FWD_LD(k) lr[(k) * 64]
            if (V != GSR_SURFEL) {
                const float4 q0 = FWD_LD(0), q1 = FWD_LD(1), q2 = FWD_LD(2);
                const float dx = q0.x - pxf, dy = q0.y - pyf;
                const float power = -0.5f * (q0.z * dx * dx + q1.x * dy * dy) - q0.w * dx * dy;
                const float alpha = fminf(0.99f, q1.y * __expf(power));
                uint64_t okm = live & __builtin_amdgcn_fcmpf(power, 0.0f, 13) & __builtin_amdgcn_fcmpf(alpha, 1.0f / 255.0f, 11);
                const float test_T = T * (1 - alpha);
                const uint64_t stopm = okm & __builtin_amdgcn_fcmpf(test_T, 0.0001f, 4);
                live &= ~stopm; okm &= ~stopm;
                if (V == GSR_PLANE) {
                    const uint64_t ob = okm & __builtin_amdgcn_fcmpf(T, 0.5f, 2);
                    if (ob != 0 && lane == 0) atomicAdd(&p.out_observe[__builtin_amdgcn_readlane((int)id, (int)sl)], (int)__popcll(ob));
                }
                const bool ok = __builtin_amdgcn_inverse_ballot_w64(okm);
                if (ok) {
                    const float w = alpha * T;
                    C0 += q1.z * w; C1 += q1.w * w; C2 += q2.x * w;
                    if (V == GSR_PLANE && p.render_geo) {
                        const float4 q3 = FWD_LD(3);
                        A0 += q2.y * w; A1 += q2.z * w; A2 += q2.w * w; A3 += q3.x * w; A4 += q3.y * w;
                    }
                    T = test_T;
                    slot_last = sl;
                }
            } else {
                const float4 q0 = FWD_LD(0), q1 = FWD_LD(1), q2 = FWD_LD(2), q3 = FWD_LD(3), q4 = FWD_LD(4);
                // p = P0 + dx Px + dy Py, (dx, dy) = this lane's pixel inside the sub-tile (staged layout: see the staging block above)
                const float ppx = fmaf(fdy, q1.z, fmaf(fdx, q0.w, q0.x)), ppy = fmaf(fdy, q1.w, fmaf(fdx, q1.x, q0.y)), ppz = fmaf(fdy, q2.x, fmaf(fdx, q1.y, q0.z));
                const float rpz = rcp_nr(ppz);
                const float sx = ppx * rpz, sy = ppy * rpz;
                const float rho3d = sx * sx + sy * sy;
                const float dx = q3.x - fdx, dy = q3.y - fdy;
                const float rho2d = FILTER_INV_SQ * (dx * dx + dy * dy);
                const float rho = fminf(rho3d, rho2d);
                const float depth = (rho3d <= rho2d) ? q2.y * rpz : q2.z;
                const float alpha = fminf(0.99f, q2.w * __builtin_amdgcn_exp2f(rho * (-0.5f * 1.4426950408889634f)));      // exp(-rho / 2)
                // (the reference's `power > 0` gate, forward.cu:389, cannot fire: rho is a minimum of two sums of squares)
                uint64_t okm = live & __builtin_amdgcn_fcmpf(ppz, 0.0f, 14) & __builtin_amdgcn_fcmpf(depth, NEAR_N, 11) & __builtin_amdgcn_fcmpf(alpha, 1.0f / 255.0f, 11);
                const float test_T = T * (1 - alpha);
                const uint64_t stopm = okm & __builtin_amdgcn_fcmpf(test_T, 0.0001f, 4);
                live &= ~stopm; okm &= ~stopm;
                const bool ok = __builtin_amdgcn_inverse_ballot_w64(okm);
                if (ok) {
                    const float w = alpha * T;
                    const float A = 1 - T;
                    const float mm = fmaf(-(FAR_N * NEAR_N) / (FAR_N - NEAR_N), rcp_(depth), FAR_N / (FAR_N - NEAR_N));      // far / (far - near) (1 - near / depth)
                    distortion += (mm * mm * A + M2 - 2 * mm * M1) * w;
                    Dd += depth * w; M1 += mm * w; M2 += mm * mm * w;
                    if (T > 0.5f) { median_depth = depth; slot_med = sl; }
                    N0 += q3.z * w; N1 += q3.w * w; N2 += q4.x * w;
                    C0 += q4.y * w; C1 += q4.z * w; C2 += q4.w * w;
                    T = test_T;
                    slot_last = sl;
                }
            }
        }
        // per batch: slots -> positions in the tile's list (1-based), and the median splat's normal and id copied from its staged record and its lane
        const uint32_t first = base - range.x + 1u;
        if (slot_last != NONE) last_contributor = first + slot_last;
        if (V == GSR_SURFEL) {
            const int mid = __builtin_amdgcn_ds_bpermute((int)((slot_med & 63u) << 2), (int)id);      // lane slot_med's id; every lane takes part, only the lanes below use it
            if (slot_med != NONE) {
                const float4* mr = s_rec + wave * ST * 64 + (slot_med & 63u);
                const float4 q3 = mr[3 * 64], q4 = mr[4 * 64];
                mn0 = q3.z; mn1 = q3.w; mn2 = q4.x;
                surf_idx = mid;
                median_contributor = first + slot_med;
            }
        }
    }

    if (inside) {
        p.final_T[pix_id] = T;
        p.n_contrib[pix_id] = last_contributor;
        p.out_color[0 * HW + pix_id] = C0 + T * p.bg[0];
        p.out_color[1 * HW + pix_id] = C1 + T * p.bg[1];
        p.out_color[2 * HW + pix_id] = C2 + T * p.bg[2];
        if (V == GSR_SURFEL) {
            p.n_contrib[pix_id + HW] = median_contributor;
            p.final_T[pix_id + HW] = M1;
            p.final_T[pix_id + 2 * HW] = M2;
            float* o = p.out_others;
            o[pix_id + 0 * HW] = Dd;
            o[pix_id + 1 * HW] = 1 - T;
            o[pix_id + 2 * HW] = N0; o[pix_id + 3 * HW] = N1; o[pix_id + 4 * HW] = N2;
            o[pix_id + 5 * HW] = median_depth;
            o[pix_id + 6 * HW] = distortion;
            o[pix_id + 7 * HW] = (float)surf_idx;
            o[pix_id + 8 * HW] = mn0; o[pix_id + 9 * HW] = mn1; o[pix_id + 10 * HW] = mn2;
        }
        if (V == GSR_PLANE && p.render_geo) {
            p.out_all_map[0 * HW + pix_id] = A0; p.out_all_map[1 * HW + pix_id] = A1; p.out_all_map[2 * HW + pix_id] = A2;
            p.out_all_map[3 * HW + pix_id] = A3; p.out_all_map[4 * HW + pix_id] = A4;
            const float rayx = (pxf - (float)(p.W * 0.5f)) / p.fx, rayy = (pyf - (float)(p.H * 0.5f)) / p.fy;
            p.out_plane_depth[pix_id] = (float)(A4 / -(double)((A0 * rayx + A1 * rayy + A2) + 1.0e-8));
        }
    }
}

// =================================================================================================== launchers
static BlendParams make_bp(const gsr_cfg* cfg, GeomView g, BinView b, ImgView im, hipStream_t s)
{
    BlendParams p = {};
    p.W = cfg->W; p.H = cfg->H;
    p.gx = (cfg->W + GSR_TILE - 1) / GSR_TILE; p.gy = (cfg->H + GSR_TILE - 1) / GSR_TILE;
    p.variant = cfg->variant; p.render_geo = cfg->render_geo;
    // Which tile workgroup b works on (it runs on XCD b % 8, every XCD has its own L2): 4x4-tile blocks dealt out to the XCDs cyclically
    // (gsr_static_tile_map) -- a block's tiles share an L2, every image region is spread over all eight XCDs; raster order (b = tile) while the map
    // is unavailable.  (One contiguous band of tiles per XCD, rounds 1-3, had the best L2 reuse but left the busy band of a non-uniform scene to
    // one XCD: 701 vs 1070 it/s with half of the gaussians in the image centre; removed in round 7.)
    p.static_map = gsr_static_tile_map(p.gx, p.gy, s);
    p.fy = cfg->H / (2.0f * cfg->tanfovy);
    p.fx = cfg->W / (2.0f * cfg->tanfovx);
    p.tile_order = im.tile_order;         // used when its word T is set: decided per forward (FwdPlan::tile_order)
    p.long_word = nullptr; p.long_len = 0xFFFFFFFFu; p.status = nullptr; p.status_total = nullptr; p.status_cap = 0u;
    p.qmask = b.qmask;                    // the forward's per-(batch, quadrant) cull ballots, read by the splat-parallel backward
    p.ranges = im.ranges; p.point_list = b.point_list; p.cull = g.cull; p.rec = g.rec; p.bg = cfg->bg;
    p.zero_rec = nullptr;
    p.depth_key = nullptr; p.list_rw = nullptr; p.tile_keys = nullptr; p.scratch_keys = nullptr; p.scratch_ids = nullptr;
    p.sort_buckets = 1; p.list_any_order = 0;
    p.final_T = im.final_T; p.n_contrib = im.n_contrib;
    return p;
}

int gsr_launch_blend_fwd(const gsr_cfg* cfg, const gsr_inputs* in, GeomView g, BinView b, ImgView im,
                         const gsr_outputs* out, hipStream_t s, const FwdPlan& plan, uint32_t* status_dev, uint32_t status_cap)
{
    (void)in;
    BlendParams p = make_bp(cfg, g, b, im, s);
    if (status_dev) { p.status = status_dev; p.status_total = g.counters; p.status_cap = status_cap; }
    if (!plan.global_order) {
        p.depth_key = g.depth_key; p.list_rw = b.point_list; p.tile_keys = b.tile_keys; p.scratch_keys = b.keys_b; p.scratch_ids = b.vals_b;
        p.list_any_order = plan.bucket_chunk ? 1 : 0;
    }
    {   // long-list feedback for the launch order of the forwards that follow (FwdPlan::tile_order): "long" = beyond max(1024, ~4 x the mean list,
        // the mean taken as 5 instances per gaussian over T tiles)
        const long long T = (long long)p.gx * p.gy;
        p.long_word = gsr_long_list_word();
        p.long_len = (uint32_t)std::max(1024ll, 20ll * (long long)cfg->P / std::max(T, 1ll));
    }
    p.out_color = out->out_color; p.out_others = out->out_others; p.out_observe = out->out_observe;
    p.out_all_map = out->out_all_map; p.out_plane_depth = out->out_plane_depth;
    dim3 grid(p.gx * p.gy), block(256);
    switch (cfg->variant) {
    case GSR_EWA: hipLaunchKernelGGL(k_blend_fwd<GSR_EWA>, grid, block, 0, s, p); break;
    case GSR_PLANE: hipLaunchKernelGGL(k_blend_fwd<GSR_PLANE>, grid, block, 0, s, p); break;
    default: hipLaunchKernelGGL(k_blend_fwd<GSR_SURFEL>, grid, block, 0, s, p); break;
    }
    return gsr_check_launch("blend_fwd", s, cfg->debug);
}

int gsr_launch_blend_bwd(const gsr_cfg* cfg, const gsr_inputs* in, GeomView g, BinView b, ImgView im,
                         const gsr_out_grads* og, float* acc, hipStream_t s)
{
    (void)in;
    BlendParams p = make_bp(cfg, g, b, im, s);
    p.dL_dcolor = og->dL_dcolor; p.dL_dothers = og->dL_dothers; p.dL_dout_all_map = og->dL_dout_all_map;
    p.dL_dplane_depth = og->dL_dplane_depth; p.all_map_pixels = og->all_map_pixels;
    p.acc = acc;
    // the splat-parallel backward of gsr_blend_sp.hip.  (Round 1's pixel-parallel kernel stayed switchable until round 7; last measured on MI355X, 300k splats,
    // 1080p in round 2: surfel sp 0.486 / px 0.524 ms, EWA 0.390 / 0.483, PLANE 0.331 / 0.372 -- DESIGN.md section 4.)
    if (gsr_launch_blend_bwd_sp(p, cfg->variant, s)) return 1;
    return gsr_check_launch("blend_bwd_sp", s, cfg->debug);
}
