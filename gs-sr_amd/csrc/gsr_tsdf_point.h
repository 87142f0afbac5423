// gsr_tsdf_point.h -- the per-point TSDF rule of compute_unbounded_tsdf (gssr/utils/mesh_utils.py:195-246) and its bilinear fetches, shared by
// gsr_extra.hip (gsr_tsdf_integrate: one frame, state in memory) and gsr_unbounded.hip (all frames fused, state in registers).  Both units are built
// without FMA contraction (PRE_FLAGS), so the two give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// torch.nn.functional.grid_sample(mode='bilinear', padding_mode='border', align_corners=True), one sample.
// Coordinates are clamped to [0, size-1]; corner weights as ATen: (x1 - x), (x - x0); out-of-range corners add 0.
__device__ __forceinline__ float bilinear_border(const float* __restrict__ img, int W, int H, float u, float v)
{
    float x = ((u + 1.f) / 2.f) * (float)(W - 1);
    float y = ((v + 1.f) / 2.f) * (float)(H - 1);
    x = fminf(fmaxf(x, 0.f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = x - (float)x0, wy1 = y - (float)y0, wx0 = (float)x1 - x, wy0 = (float)y1 - y;
    float acc = 0.f;
    if (x0 < W && y0 < H) acc += img[(size_t)y0 * W + x0] * (wx0 * wy0);
    if (x1 < W && y0 < H) acc += img[(size_t)y0 * W + x1] * (wx1 * wy0);
    if (x0 < W && y1 < H) acc += img[(size_t)y1 * W + x0] * (wx0 * wy1);
    if (x1 < W && y1 < H) acc += img[(size_t)y1 * W + x1] * (wx1 * wy1);
    return acc;
}

// same clamping, weights and corner order as bilinear_border, on all four channels at once (bit-identical per channel)
__device__ __forceinline__ float4 bilinear_border4(const float4* __restrict__ img, int W, int H, float u, float v)
{
    float x = ((u + 1.f) / 2.f) * (float)(W - 1);
    float y = ((v + 1.f) / 2.f) * (float)(H - 1);
    x = fminf(fmaxf(x, 0.f), (float)(W - 1));
    y = fminf(fmaxf(y, 0.f), (float)(H - 1));
    const int x0 = (int)floorf(x), y0 = (int)floorf(y);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const float wx1 = x - (float)x0, wy1 = y - (float)y0, wx0 = (float)x1 - x, wy0 = (float)y1 - y;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto add = [&](int xx, int yy, float w) {
        if (xx < W && yy < H) {
            const float4 t = img[(size_t)yy * W + xx];
            acc.x += t.x * w; acc.y += t.y * w; acc.z += t.z * w; acc.w += t.w * w;
        }
    };
    add(x0, y0, wx0 * wy0); add(x1, y0, wx1 * wy0); add(x0, y1, wx0 * wy1); add(x1, y1, wx1 * wy1);
    return acc;
}

// One sample point: the update of compute_unbounded_tsdf (mesh_utils.py:208-246), the ONE statement of the rule.  Returns true when the voxel changed.
// COLOUR = false: the caller keeps no colour state (the lattice pass: the reference's sdf callable discards rgb); rgb / rgbd / col are not touched, and
// tsdf and weight go through the same operations, so they take the same bits.
template <bool COLOUR>
__device__ __forceinline__ bool tsdf_point_rule(const float* F, float x, float y, float z3, int W, int H, const float* __restrict__ depth,
                                                const float* __restrict__ rgb, const float4* __restrict__ rgbd, float tr, float& tsdf,
                                                float& weight, float* col /*[3]*/)
{
    const float qx = x * F[0] + y * F[4] + z3 * F[8] + F[12];
    const float qy = x * F[1] + y * F[5] + z3 * F[9] + F[13];
    const float qw = x * F[3] + y * F[7] + z3 * F[11] + F[15];
    const float u = qx / qw, v = qy / qw;
    bool mask = (u > -1.f) && (u < 1.f) && (v > -1.f) && (v < 1.f) && (qw > 0);
    if (!mask) return false;                      // the reference samples depth for every point; the result is masked anyway
    float4 tex;
    if (COLOUR && rgbd) tex = bilinear_border4(rgbd, W, H, u, v);
    else tex.w = bilinear_border(depth, W, H, u, v);
    const float sdf = tex.w - qw;
    if (!(sdf > -tr)) return false;
    if (COLOUR && !rgbd) {
        const size_t HW = (size_t)W * H;
        tex.x = bilinear_border(rgb, W, H, u, v); tex.y = bilinear_border(rgb + HW, W, H, u, v); tex.z = bilinear_border(rgb + 2 * HW, W, H, u, v);
    }
    float s = sdf / tr;
    s = fminf(fmaxf(s, -1.0f), 1.0f);
    const float w = weight, wp = w + 1;
    tsdf = (tsdf * w + s) / wp;
    if (COLOUR) { col[0] = (col[0] * w + tex.x) / wp; col[1] = (col[1] * w + tex.y) / wp; col[2] = (col[2] * w + tex.z) / wp; }
    weight = wp;
    return true;
}
__device__ __forceinline__ bool tsdf_point(const float* F, float x, float y, float z3, int W, int H, const float* __restrict__ depth,
                                           const float* __restrict__ rgb, const float4* __restrict__ rgbd, float tr, float& tsdf,
                                           float& weight, float* col /*[3]*/)
{
    return tsdf_point_rule<true>(F, x, y, z3, W, H, depth, rgb, rgbd, tr, tsdf, weight, col);
}
__device__ __forceinline__ bool tsdf_point_depth(const float* F, float x, float y, float z3, int W, int H, const float* __restrict__ depth, float tr,
                                                 float& tsdf, float& weight)
{
    return tsdf_point_rule<false>(F, x, y, z3, W, H, depth, nullptr, nullptr, tr, tsdf, weight, nullptr);
}
