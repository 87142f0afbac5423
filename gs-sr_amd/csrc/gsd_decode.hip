// gsd_decode.hip -- fused neural-Gaussian decode (include/gsdecode.h), gfx950 only.
//
// Reference behaviour: ScaffoldScene/OctreeScene.generate_neural_gaussians (gssr/scene/scaffold_scene.py:27-120,
// gssr/scene/octree_scene.py:26-133) -- ~60 torch ops + autograd; here 2 forward kernels and 3 backward kernels.
//
// Mapping to the hardware
//   * forward / per-anchor backward: one lane = one visible anchor, 64 anchors per wave.  The three heads are 32-wide MLPs whose weights
//     are identical for every lane, so they are fetched with SCALAR loads (constant address space -> s_load_dwordx8/16 into SGPRs) and
//     used directly as the SGPR operand of v_fmac: no LDS, no VGPRs for weights, the per-anchor state (x[37], h[32], dh[32], dx[37])
//     stays in registers.  fp32 MFMA has the same peak as packed fp32 FMA on CDNA4, so MFMA buys nothing for these lane-local products.
//   * weight gradients: dW = sum over anchors of (dpre x^T) IS a contraction across lanes, i.e. exactly what MFMA does.  The per-anchor
//     kernel stores x, h and the pre-activation gradients feature-major ([column][anchor], coalesced); k_wgrad then runs
//     v_mfma_f32_16x16x4_f32 with the anchor index as the K dimension (operands are plain float4 loads, 16 consecutive anchors of one
//     column per lane), split-K over persistent waves, followed by a small deterministic reduction of the partial tiles.
//   * layer-1 weights are first repacked (k_pack) to a fixed [head][32][48] layout: columns feat 0..31, view 32..34, dist 35, level 36,
//     effective bias 37 (b1 + W1[:, appearance cols] . appearance) -- absent inputs get zero weights, so the hot kernels carry no flags.
#include "gsr_common.h"
#include "gsr_reduce.h"
#include "gsr_scan.h"
#include "../../include/gsdecode.h"

#define GSD_XC 37            // x = [feat 32, view 3, dist, level]
#define GSD_W1LD 48          // packed layer-1 row stride (floats); column 37 = effective bias
#define GSD_W1P_FLOATS (3 * 32 * GSD_W1LD)
#define GSD_BLOCK 256

typedef const float __attribute__((address_space(4))) * cfp;     // constant address space: wave-uniform index -> scalar load
#define CW(p) ((cfp)(p))

// column blocks of the backward scratch.  Layout is TILE-major: element (column c, anchor v) lives at ((v/16)*SC_COLS + c)*16 + v%16,
// so the 16-anchor tile a wave produces is one contiguous 26 KB block (a column-major [c][Nv] layout made every wave stream into
// 416 different pages and ran the producer at <0.6 TB/s), and k_wgrad still reads 16 consecutive anchors of a column as 4 float4.
#define SC_X 0               // 48 (37 used)
#define SC_H 48              // 3 x 32
#define SC_P1 144            // dpre1: 3 x 32
#define SC_P2O 240           // dpre2 opacity: 16
#define SC_P2K 256           // dpre2 colour: 48
#define SC_P2C 304           // dpre2 cov: 112
#define SC_COLS 416

#define WG_WAVES 128         // persistent waves per weight-gradient problem
#define WG_MAXPROB 24

struct DecArgs {
    gsd_cfg cfg;
    gsd_inputs in;
};

// ------------------------------------------------------------------------------------------------ small device helpers
__device__ __forceinline__ float sigmoid_(float x) { return 1.0f / (1.0f + __expf(-x)); }

// ------------------------------------------------------------------------------------------------ scan (exclusive, in place)
// Exclusive scan of data[0, n) in place, one launch, no ticket: every workgroup scans its 1024 words, PUBLISHES its total (flag word = ready bit |
// total) and then adds up the published totals of all workgroups in front of it -- one load per predecessor, spinning on the ready bits.  Workgroups
// are dispatched in index order and only ever wait for lower indices, so the wait ends; nobody waits in a chain (each total is published before its
// workgroup looks back).  CONTRACT: flags[0, gridDim.x) must be ZERO at launch -- the kernel in front of this one clears them (k_pack_img / k_flags: every
// caller of launch_scan below launches one of the two right in front of it); stale ready bits of an earlier run would be read as this run's totals.
// The last workgroup writes the grand total.  (Rounds 2-3 had a ticket counter instead -- the workgroup that drew the last ticket scanned the block
// sums, a third kernel added them: 59 atomics on one word cost 8.9 us, 0.15 us each, plus the 3.9 us of k_scan_add; DESIGN Appendix A (70).)
#define GSD_SCAN_READY 0x80000000u
#define GSD_SCAN_POISON 0xFFFFFFFFu      // *total when the look-back gave up: no real total reaches 2^31 (the ready bit); the host entry points check for it
#define GSD_SCAN_TIMEOUT_MSG "the scan's look-back timed out (a workgroup in front never published its total: workgroups not dispatched in index order?)"
#define GSD_SCAN_SPINS (1u << 21)       // x s_sleep 8 (~0.5 us): ~1 s.  A predecessor publishes its total ~2 us after it starts
__global__ void __launch_bounds__(1024) k_scan_lookback(uint32_t* __restrict__ data, uint32_t n, uint32_t* __restrict__ flags, uint32_t* __restrict__ total)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t s_prev;
    const uint32_t i = blockIdx.x * 1024u + threadIdx.x;
    const uint32_t v = i < n ? data[i] : 0u;
    const uint32_t incl = wave_incl_scan(v);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
    for (int w = 0; w < 16; w++) { if (w < wave) base += wsum[w]; all += wsum[w]; }
    if (threadIdx.x == 0) __hip_atomic_store(&flags[blockIdx.x], GSD_SCAN_READY | all, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    // The look-back is ONE wave's job (all 1024 threads used to spin): lane l adds the totals of predecessors l, l + 64, ...  The wait relies on
    // workgroups being DISPATCHED in index order (a workgroup only waits for lower indices, and every workgroup publishes before it looks back, so a
    // resident predecessor always gets there) -- what the hardware's dispatcher does for a 1-D grid, but not an API guarantee: the spin is bounded, and a
    // wave that gives up poisons the total instead of hanging the device (the callers turn GSD_SCAN_POISON into an error).
    if (wave == 0) {
        uint32_t back = 0;
        bool gave_up = false;
        for (uint32_t q = (uint32_t)lane; q < blockIdx.x && !gave_up; q += 64u) {
            uint32_t f, spins = 0;
            while (!((f = __hip_atomic_load(&flags[q], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) & GSD_SCAN_READY)) {
                if (++spins > GSD_SCAN_SPINS) { gave_up = true; break; }
                __builtin_amdgcn_s_sleep(8);
            }
            back += f & ~GSD_SCAN_READY;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) back += (uint32_t)__shfl_xor((int)back, d, 64);
        // a predecessor that never publishes stops EVERY workgroup behind it, the last one included: the last workgroup's verdict is the launch's
        if (__ballot(gave_up) != 0ull) back = GSD_SCAN_POISON;
        if (lane == 0) s_prev = back;
    }
    __syncthreads();
    const uint32_t prev = s_prev;
    // a workgroup that gave up writes an IN-RANGE sentinel (position 0), not POISON + offset: the kernels queued behind the scan (k_scatter_idx, the stage-2
    // emitters: `out[pos[i]]`, `row_offset[i]`) run before any host could look at the total, and must stay inside their buffers
    if (i < n) data[i] = (prev == GSD_SCAN_POISON) ? 0u : prev + base + incl - v;
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = (prev == GSD_SCAN_POISON) ? GSD_SCAN_POISON : prev + all;
}
// data[0..n) -> exclusive prefix in place, *total_dev = sum.  flags: >= div_up(n,1024) words, zeroed by the kernel in front (k_flags).
static void launch_scan(uint32_t* data, uint32_t n, uint32_t* flags, uint32_t* total_dev, hipStream_t s)
{
    hipLaunchKernelGGL(k_scan_lookback, dim3(gsr_div_up(n, 1024u)), dim3(1024), 0, s, data, n, flags, total_dev);
}

__global__ void __launch_bounds__(256) k_flags(const uint8_t* __restrict__ mask, uint32_t n, uint32_t* __restrict__ flags, uint32_t* __restrict__ scan_flags,
                                               uint32_t n_scan_flags)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_scan_flags) scan_flags[i] = 0u;           // k_scan_lookback's ready words (n_scan_flags = ceil(n / 1024) <= the threads of this grid)
    if (i < n) flags[i] = mask[i] ? 1u : 0u;
}
__global__ void __launch_bounds__(256) k_scatter_idx(const uint8_t* __restrict__ mask, uint32_t n, const uint32_t* __restrict__ pos,
                                                     int32_t* __restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && mask[i]) out[pos[i]] = (int32_t)i;
}

// ------------------------------------------------------------------------------------------------ weight image (MFMA operand order)
// v_mfma_f32_16x16x4_f32: lane l = (i = l & 15, kk = l >> 4) supplies A[m = i][k = kk] and B[k = kk][n = i]; it receives
// D[m = 4 kk + r][n = i] in acc[r].  All activations are kept TRANSPOSED, as [feature][anchor] tiles in D layout (16 anchors per
// tile on i, feature 16 t + 4 kk + r on (t, kk, r)), so that the output tile of one layer is directly the B operand of the next:
// at contraction step (t, r) lane (i, kk) contributes feature 16 t + 4 kk + r and the weight operand must hold W[m][16 t + 4 kk + r].
// k_pack_img writes every weight operand of forward and backward in exactly that per-lane order ("slots" of 64 floats); the kernels
// copy the slots they need into LDS once per block and read them with conflict-free ds_read_b32.
//   layer-2 output rows are re-grouped so that the epilogue is lane-local: cov head 8 rows per offset (7 used) -> lane (kk even) holds
//   (s0,s1,s2,q0), lane kk+1 holds (q1,q2,q3,-) of offset 2 ot + kk/2; colour head 4 rows per offset (3 used) -> lane kk holds offset
//   4 ot + kk; opacity head: lane kk holds offsets 4 kk .. 4 kk + 3.
#define IMG_W1F 0        // [h 3][ht 2][t 3][r 4]     A[m = hidden][k = x column]
#define IMG_W2F_O 72     // [ht 2][r 4]               A[m = out row][k = hidden]
#define IMG_W2F_C 80     // [ot 8][ht 2][r 4]
#define IMG_W2F_K 144    // [ot 4][ht 2][r 4]
#define IMG_B2_O 176     // [r 4]                     bias in D layout
#define IMG_B2_C 180     // [ot 8][r 4]
#define IMG_B2_K 212     // [ot 4][r 4]
#define IMG_W2T_O 228    // [ht 2][r 4]               A[m = hidden][k = out row]
#define IMG_W2T_C 236    // [ht 2][ot 8][r 4]
#define IMG_W2T_K 300    // [ht 2][ot 4][r 4]
#define IMG_W1T 332      // [h 3][xt 3][ht 2][r 4]    A[m = x column][k = hidden]
#define IMG_SLOTS 404
#define IMG_FLOATS (IMG_SLOTS * 64)

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct PackArgs {
    gsd_cfg cfg;
    const float *W1o, *b1o, *W2o, *b2o, *W1c, *b1c, *W2c, *b2c, *W1k, *b1k, *W2k, *b2k, *app;
    float* img;
    uint32_t* scan_flags; uint32_t n_scan_flags;       // k_scan_lookback's ready words to clear (or NULL, 0)
};

// packed layer-1 weight: columns feat 0..31, view 32..34, dist 35, level 36, 37 = bias + appearance contribution, 38.. = 0
__device__ float w1p(const PackArgs& p, int head, int j, int c)
{
    const int lv = p.cfg.level ? 1 : 0;
    const float* W = head == 0 ? p.W1o : (head == 1 ? p.W1c : p.W1k);
    const float* b = head == 0 ? p.b1o : (head == 1 ? p.b1c : p.b1k);
    const int dist = head == 0 ? p.cfg.dist_o : (head == 1 ? p.cfg.dist_c : p.cfg.dist_k);
    const int A = head == 2 ? p.cfg.A : 0;
    const int in = 35 + (dist ? 1 : 0) + lv + A;
    if (c < 35) return W[j * in + c];
    if (c == 35) return dist ? W[j * in + 35] : 0.0f;
    if (c == 36) return lv ? W[j * in + 35 + (dist ? 1 : 0)] : 0.0f;
    if (c == GSD_XC) {
        float v = 0.0f;
        const int base = 35 + (dist ? 1 : 0) + lv;
        for (int i = 0; i < A; i++) v = fmaf(W[j * in + base + i], p.app[i], v);       // appearance is the same for every anchor
        return v + b[j];
    }
    return 0.0f;
}
// layer-2 rows in the re-grouped order: head 0: rho = offset; head 1: rho = 8 j + c (c < 7); head 2: rho = 4 j + c (c < 3)
__device__ float w2row(const PackArgs& p, int head, int rho, int hid, bool bias)
{
    const int k = p.cfg.k;
    int j, c, per;
    if (head == 0) { j = rho; c = 0; per = 1; }
    else if (head == 1) { j = rho >> 3; c = rho & 7; per = 7; }
    else { j = rho >> 2; c = rho & 3; per = 3; }
    if (j >= k || c >= per) return 0.0f;
    const int row = per * j + c;
    const float* W = head == 0 ? p.W2o : (head == 1 ? p.W2c : p.W2k);
    const float* b = head == 0 ? p.b2o : (head == 1 ? p.b2c : p.b2k);
    return bias ? b[row] : W[row * 32 + hid];
}

__global__ void __launch_bounds__(256) k_pack_img(PackArgs p)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    for (uint32_t z = (uint32_t)e; z < p.n_scan_flags; z += gridDim.x * 256u) p.scan_flags[z] = 0u;
    if (e >= IMG_FLOATS) return;
    const int slot = e >> 6, l = e & 63, m = l & 15, kk = l >> 4;
    float v;
    if (slot < IMG_W2F_O) {
        const int s = slot - IMG_W1F, r = s & 3, t = (s >> 2) % 3, ht = (s / 12) & 1, h = s / 24;
        v = w1p(p, h, 16 * ht + m, 16 * t + 4 * kk + r);
    } else if (slot < IMG_B2_O) {
        int head, s;
        if (slot < IMG_W2F_C) { head = 0; s = slot - IMG_W2F_O; }
        else if (slot < IMG_W2F_K) { head = 1; s = slot - IMG_W2F_C; }
        else { head = 2; s = slot - IMG_W2F_K; }
        const int r = s & 3, ht = (s >> 2) & 1, ot = s >> 3;
        v = w2row(p, head, 16 * ot + m, 16 * ht + 4 * kk + r, false);
    } else if (slot < IMG_W2T_O) {
        int head, s;
        if (slot < IMG_B2_C) { head = 0; s = slot - IMG_B2_O; }
        else if (slot < IMG_B2_K) { head = 1; s = slot - IMG_B2_C; }
        else { head = 2; s = slot - IMG_B2_K; }
        const int r = s & 3, ot = s >> 2;
        v = w2row(p, head, 16 * ot + 4 * kk + r, 0, true);
    } else if (slot < IMG_W1T) {
        int head, s, not_;
        if (slot < IMG_W2T_C) { head = 0; s = slot - IMG_W2T_O; not_ = 1; }
        else if (slot < IMG_W2T_K) { head = 1; s = slot - IMG_W2T_C; not_ = 8; }
        else { head = 2; s = slot - IMG_W2T_K; not_ = 4; }
        const int r = s & 3, ot = (s >> 2) % not_, ht = (s >> 2) / not_;
        v = w2row(p, head, 16 * ot + 4 * kk + r, 16 * ht + m, false);
    } else {
        const int s = slot - IMG_W1T, r = s & 3, ht = (s >> 2) & 1, xt = (s >> 3) % 3, h = s / 24;
        const int col = 16 * xt + m;
        v = col < GSD_XC ? w1p(p, h, 16 * ht + 4 * kk + r, col) : 0.0f;
    }
    p.img[e] = v;
}

// copy `count` consecutive slots of the global image into LDS (dst slot index given), all threads of the block
__device__ __forceinline__ void img_to_lds(float* lds, int dst_slot, const float* __restrict__ img, int src_slot, int count)
{
    const float4* s = reinterpret_cast<const float4*>(img + (size_t)src_slot * 64);
    float4* d = reinterpret_cast<float4*>(lds + (size_t)dst_slot * 64);
    for (int i = threadIdx.x; i < count * 16; i += blockDim.x) d[i] = s[i];
}

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// B-operand tiles of x = [feat 32 | view 3, dist | level, 1, 0, 0 | 0...] for anchor `a` (all zero for padding anchors)
// Row v of the visible-anchor list: anchor index, or "inactive" for rows past Nv AND for padding rows (vis_idx[v] < 0).  The padded form
// (gsd_compact_visible_padded: vis_idx has Na entries, -1 behind the visible ones, Nv = Na) lets the caller enqueue the decode without
// first reading the number of visible anchors back to the host.
__device__ __forceinline__ bool row_anchor(const int32_t* __restrict__ vis_idx, int v, int Nv, int& a)
{
    const int a0 = v < Nv ? vis_idx[v] : -1;
    a = a0 >= 0 ? a0 : 0;
    return a0 >= 0;
}
__device__ __forceinline__ void load_xb(const DecArgs& p, int a, bool active, int kk, f32x4 (&xb)[3], float (&vw)[3], float& dist)
{
    const float4* f4 = reinterpret_cast<const float4*>(p.in.feat + (size_t)a * GSD_FEAT);
    const float4 f0 = f4[kk], f1 = f4[4 + kk];
    const float r0 = p.in.anchor[3 * a] - p.in.campos[0], r1 = p.in.anchor[3 * a + 1] - p.in.campos[1],
                r2 = p.in.anchor[3 * a + 2] - p.in.campos[2];
    dist = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
    vw[0] = r0 / dist; vw[1] = r1 / dist; vw[2] = r2 / dist;
    const float lv = p.in.level ? p.in.level[a] : 0.0f;
    // inactive rows read anchor 0, which need not be finite (at the camera centre its view vector is 0/0): SELECT zeros, never multiply by 0 -- a NaN
    // column in the scratch poisons the weight-gradient contraction over anchors (0 x NaN)
    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    xb[0] = active ? (f32x4){f0.x, f0.y, f0.z, f0.w} : zero;
    xb[1] = active ? (f32x4){f1.x, f1.y, f1.z, f1.w} : zero;
    xb[2] = !active ? zero : (kk == 0 ? (f32x4){vw[0], vw[1], vw[2], dist} : (kk == 1 ? (f32x4){lv, 1.0f, 0.0f, 0.0f} : zero));
}

// pre1^T tiles of one head: acc[ht][r] = pre-activation of hidden unit 16 ht + 4 kk + r.  w1: LDS slots [ht 2][t 3][r 4] of that head
__device__ __forceinline__ void layer1_mfma(const float* w1, int lane, const f32x4 (&xb)[3], f32x4 (&acc)[2])
{
#pragma unroll
    for (int ht = 0; ht < 2; ht++) {
        acc[ht] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 3; t++)
#pragma unroll
            for (int r = 0; r < 4; r++) acc[ht] = MFMA(w1[((ht * 3 + t) * 4 + r) * 64 + lane], xb[t][r], acc[ht]);
    }
}
// one 16-row output tile of layer 2: w2 = LDS slots [ht 2][r 4] of that tile, bias = LDS slots [r 4]
__device__ __forceinline__ f32x4 layer2_mfma(const float* w2, const float* bias, int lane, const f32x4 (&hb)[2])
{
    f32x4 y = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ht = 0; ht < 2; ht++)
#pragma unroll
        for (int r = 0; r < 4; r++) y = MFMA(w2[(ht * 4 + r) * 64 + lane], hb[ht][r], y);
#pragma unroll
    for (int r = 0; r < 4; r++) y[r] += bias[r * 64 + lane];
    return y;
}
__device__ __forceinline__ f32x4 relu4(f32x4 v) { return (f32x4){fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)}; }

__device__ __forceinline__ uint32_t mask_bits(const float* __restrict__ nop, int v, int k, bool active)
{
    uint32_t m = 0;
    if (active)
        for (int j = 0; j < k; j++) m |= nop[(size_t)v * k + j] > 0.0f ? (1u << j) : 0u;
    return m;
}

// ------------------------------------------------------------------------------------------------ forward stage 1: opacity head
// LDS: [W1F head 0: 24][W2F_O: 8][B2_O: 4]
__global__ void __launch_bounds__(GSD_BLOCK) k_dec_opacity(DecArgs p, const float* __restrict__ img, float* __restrict__ neural_opacity,
                                                           uint8_t* __restrict__ mask, uint32_t* __restrict__ counts, int n_tiles)
{
    __shared__ float lds[36 * 64];
    img_to_lds(lds, 0, img, IMG_W1F, 24);
    img_to_lds(lds, 24, img, IMG_W2F_O, 8);
    img_to_lds(lds, 32, img, IMG_B2_O, 4);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kk = lane >> 4, k = p.cfg.k;
    for (int tile = blockIdx.x * (GSD_BLOCK / 64) + wave; tile < n_tiles; tile += gridDim.x * (GSD_BLOCK / 64)) {
        const int v = tile * 16 + n;
        int a;
        const bool active = row_anchor(p.in.vis_idx, v, p.cfg.Nv, a);
        f32x4 xb[3], acc[2], hb[2];
        float vw[3], dist;
        load_xb(p, a, active, kk, xb, vw, dist);
        layer1_mfma(lds, lane, xb, acc);
        hb[0] = relu4(acc[0]); hb[1] = relu4(acc[1]);
        const f32x4 y = layer2_mfma(lds + 24 * 64, lds + 32 * 64, lane, hb);
        const float osc = p.in.opacity_scale ? p.in.opacity_scale[a] : 1.0f;
        uint32_t cnt = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int j = 4 * kk + r;
            float o = tanhf(y[r]);
            if (p.in.opacity_scale) o *= osc;
            if (active && j < k) {
                neural_opacity[(size_t)v * k + j] = o;
                mask[(size_t)v * k + j] = o > 0.0f ? 1 : 0;
                cnt += o > 0.0f ? 1u : 0u;
            } else if (v < p.cfg.Nv && j < k) {      // padding row: emits nothing
                neural_opacity[(size_t)v * k + j] = 0.0f;
                mask[(size_t)v * k + j] = 0;
            }
        }
        cnt += __shfl_xor(cnt, 16, 64);
        cnt += __shfl_xor(cnt, 32, 64);
        if (v < p.cfg.Nv && kk == 0) counts[v] = active ? cnt : 0u;
    }
}

// ------------------------------------------------------------------------------------------------ forward stage 2: cov + colour heads
// blockIdx.y = 0: cov head (+ xyz, opacity), 1: colour head.  LDS: [W1F 24][W2F 8 NOT][B2 4 NOT], NOT = 8 / 4 -> 30 KB / 18 KB
template <int HEAD>
__device__ __forceinline__ void emit_head(const DecArgs& p, const float* __restrict__ img, const float* __restrict__ neural_opacity,
                                          const uint32_t* __restrict__ row_offset, const gsd_outputs& out, int n_tiles, float* lds)
{
    constexpr int NOT = HEAD == 1 ? 8 : 4;
    constexpr int L_W2F = 24, L_B2 = L_W2F + 8 * NOT;
    img_to_lds(lds, 0, img, IMG_W1F + 24 * HEAD, 24);
    img_to_lds(lds, L_W2F, img, HEAD == 1 ? IMG_W2F_C : IMG_W2F_K, 8 * NOT);
    img_to_lds(lds, L_B2, img, HEAD == 1 ? IMG_B2_C : IMG_B2_K, 4 * NOT);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kk = lane >> 4, k = p.cfg.k;
    const int n_ot = HEAD == 1 ? (k + 1) >> 1 : (k + 3) >> 2;
    for (int tile = blockIdx.x * (GSD_BLOCK / 64) + wave; tile < n_tiles; tile += gridDim.x * (GSD_BLOCK / 64)) {
        const int v = tile * 16 + n;
        int a;
        const bool active = row_anchor(p.in.vis_idx, v, p.cfg.Nv, a);
        f32x4 xb[3], acc[2], hb[2];
        float vw[3], dist;
        load_xb(p, a, active, kk, xb, vw, dist);
        const uint32_t row0 = active ? row_offset[v] : 0u;
        const uint32_t mbits = mask_bits(neural_opacity, v, k, active);
        float S[6], A3[3];
        if (HEAD == 1) {
#pragma unroll
            for (int i = 0; i < 6; i++) S[i] = p.in.scaling[(size_t)a * 6 + i];
#pragma unroll
            for (int i = 0; i < 3; i++) A3[i] = p.in.anchor[3 * a + i];
        }
        layer1_mfma(lds, lane, xb, acc);
        hb[0] = relu4(acc[0]); hb[1] = relu4(acc[1]);
#pragma unroll 1
        for (int ot = 0; ot < n_ot; ot++) {
            const f32x4 y = layer2_mfma(lds + (L_W2F + ot * 8) * 64, lds + (L_B2 + ot * 4) * 64, lane, hb);
            if (HEAD == 1) {     // lane pair (kk even, kk odd) = (s0 s1 s2 q0 | q1 q2 q3 -) of offset 2 ot + kk/2
                const int j = 2 * ot + (kk >> 1), half = kk & 1;
                const float own = half ? (y[0] * y[0] + y[1] * y[1] + y[2] * y[2]) : (y[3] * y[3]);
                const float nn = own + __shfl_xor(own, 16, 64);
                const float q0 = __shfl_xor(y[3], 16, 64);
                if (j < k && ((mbits >> j) & 1u)) {
                    const uint32_t row = row0 + __popc(mbits & ((1u << j) - 1u));
                    if (half == 0) {
                        const float* off = p.in.offset + ((size_t)a * k + j) * 3;
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            out.xyz[(size_t)row * 3 + i] = A3[i] + off[i] * S[i];
                            out.scaling[(size_t)row * 3 + i] = S[3 + i] * sigmoid_(y[i]);
                        }
                        out.opacity[row] = neural_opacity[(size_t)v * k + j];
                    } else {
                        const float nrm = fmaxf(sqrtf(nn), 1e-12f);
                        reinterpret_cast<float4*>(out.rot)[row] = make_float4(q0 / nrm, y[0] / nrm, y[1] / nrm, y[2] / nrm);
                    }
                }
            } else {             // lane kk = offset 4 ot + kk, rows (r, g, b, -)
                const int j = 4 * ot + kk;
                if (j < k && ((mbits >> j) & 1u)) {
                    const uint32_t row = row0 + __popc(mbits & ((1u << j) - 1u));
#pragma unroll
                    for (int r = 0; r < 3; r++) out.color[(size_t)row * 3 + r] = sigmoid_(y[r]);
                }
            }
        }
    }
}
__global__ void __launch_bounds__(GSD_BLOCK) k_dec_emit(DecArgs p, const float* __restrict__ img, const float* __restrict__ neural_opacity,
                                                        const uint32_t* __restrict__ row_offset, gsd_outputs out, int n_tiles)
{
    __shared__ float lds[120 * 64];
    if (blockIdx.y == 0) emit_head<1>(p, img, neural_opacity, row_offset, out, n_tiles, lds);
    else emit_head<2>(p, img, neural_opacity, row_offset, out, n_tiles, lds);
}

// ------------------------------------------------------------------------------------------------ backward, per anchor tile
// Split by head (blockIdx.y) so that each block needs only its head's operands in LDS (17 / 52 / 32 KB -> several blocks per CU) and a
// small register state: forward recompute -> lane-local layer-2 pre-activation gradients -> dH = W2^T dY -> dpre1 = dH * relu'.
// x, h, dpre1, dpre2 go to the tile-major scratch for the weight-gradient contraction (k_wgrad); k_dec_bwd_dx then forms
// dX = [W1o; W1c; W1k]^T dpre1 from the same scratch and writes the per-anchor gradients.
#define SC_AT(sc, tile, col, n) (sc)[((size_t)(tile) * SC_COLS + (col)) * 16 + (n)]
#define SC_GEO (SC_X + 38)    // 9 spare x columns: dA[3], dS[6] of the geometry, written by the cov head
__device__ __forceinline__ void store_tile(float* __restrict__ sc, int tile, int col0, int kk, int n, f32x4 t)
{
#pragma unroll
    for (int r = 0; r < 4; r++) SC_AT(sc, tile, col0 + 4 * kk + r, n) = t[r];
}

struct BwdArgs {
    DecArgs d;
    const float* img; const float* neural_opacity; const uint32_t* row_offset;
    gsd_out_grads og;
    float* d_offset; float* sc; int n_tiles;
};

// LDS slot map of one head: [W1F 24][W2F 8*NOT][B2 4*NOT][W2T 2*4*NOT][...]; NOT = 1 / 8 / 4 layer-2 row tiles
template <int HEAD>
__device__ __forceinline__ void bwd_head(const BwdArgs& p, float* lds)
{
    constexpr int NOT = HEAD == 0 ? 1 : (HEAD == 1 ? 8 : 4);
    constexpr int L_W2F = 24, L_B2 = L_W2F + 8 * NOT, L_W2T = L_B2 + 4 * NOT;
    constexpr int G_W2F = HEAD == 0 ? IMG_W2F_O : (HEAD == 1 ? IMG_W2F_C : IMG_W2F_K);
    constexpr int G_B2 = HEAD == 0 ? IMG_B2_O : (HEAD == 1 ? IMG_B2_C : IMG_B2_K);
    constexpr int G_W2T = HEAD == 0 ? IMG_W2T_O : (HEAD == 1 ? IMG_W2T_C : IMG_W2T_K);
    img_to_lds(lds, 0, p.img, IMG_W1F + 24 * HEAD, 24);
    img_to_lds(lds, L_W2F, p.img, G_W2F, 8 * NOT);
    img_to_lds(lds, L_B2, p.img, G_B2, 4 * NOT);
    img_to_lds(lds, L_W2T, p.img, G_W2T, 8 * NOT);
    __syncthreads();
    const DecArgs& d = p.d;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kk = lane >> 4, k = d.cfg.k;
    const int n_ot = HEAD == 0 ? 1 : (HEAD == 1 ? (k + 1) >> 1 : (k + 3) >> 2);
    float* __restrict__ sc = p.sc;
    for (int tile = blockIdx.x * (GSD_BLOCK / 64) + wave; tile < p.n_tiles; tile += gridDim.x * (GSD_BLOCK / 64)) {
        const int v = tile * 16 + n;
        int a;
        const bool active = row_anchor(d.in.vis_idx, v, d.cfg.Nv, a);
        f32x4 xb[3], acc[2], hb[2], dh[2];
        float vw[3], dist;
        load_xb(d, a, active, kk, xb, vw, dist);
        if (HEAD == 0) {
#pragma unroll
            for (int t = 0; t < 3; t++)
#pragma unroll
                for (int r = 0; r < 4; r++)
                    if (16 * t + 4 * kk + r < 38) SC_AT(sc, tile, SC_X + 16 * t + 4 * kk + r, n) = xb[t][r];
        }
        const uint32_t row0 = active ? p.row_offset[v] : 0u;
        const uint32_t mbits = mask_bits(p.neural_opacity, v, k, active);
        layer1_mfma(lds, lane, xb, acc);
        hb[0] = relu4(acc[0]); hb[1] = relu4(acc[1]);
        dh[0] = dh[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
        float S[6], dS[6] = {0, 0, 0, 0, 0, 0}, dA[3] = {0, 0, 0};
        if (HEAD == 1) {
#pragma unroll
            for (int i = 0; i < 6; i++) S[i] = d.in.scaling[(size_t)a * 6 + i];
        }
        const float osc = (HEAD == 0 && d.in.opacity_scale) ? d.in.opacity_scale[a] : 1.0f;
#pragma unroll 1
        for (int ot = 0; ot < n_ot; ot++) {
            const f32x4 y = layer2_mfma(lds + (L_W2F + ot * 8) * 64, lds + (L_B2 + ot * 4) * 64, lane, hb);
            f32x4 g = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (HEAD == 0) {                 // opacity = tanh(.) * scale; lane kk = offsets 4 kk .. 4 kk + 3
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = 4 * kk + r;
                    if (j < k && ((mbits >> j) & 1u)) {
                        const uint32_t row = row0 + __popc(mbits & ((1u << j) - 1u));
                        const float t = tanhf(y[r]);
                        g[r] = p.og.opacity[row] * osc * (1.0f - t * t);
                    }
                }
                store_tile(sc, tile, SC_P2O, kk, n, g);
            } else if (HEAD == 1) {          // lane pair = (s0 s1 s2 q0 | q1 q2 q3 -) of offset 2 ot + kk/2; also xyz = anchor + offset*S[0:3]
                const int j = 2 * ot + (kk >> 1), half = kk & 1;
                const bool m = j < k && ((mbits >> j) & 1u);
                const uint32_t row = row0 + __popc(mbits & ((1u << j) - 1u));
                float4 gr = make_float4(0.f, 0.f, 0.f, 0.f);
                if (m) gr = reinterpret_cast<const float4*>(p.og.rot)[row];
                const float own_sq = half ? (y[0] * y[0] + y[1] * y[1] + y[2] * y[2]) : (y[3] * y[3]);
                const float own_dot = half ? (y[0] * gr.y + y[1] * gr.z + y[2] * gr.w) : (y[3] * gr.x);
                const float nn = own_sq + __shfl_xor(own_sq, 16, 64);
                const float qd = own_dot + __shfl_xor(own_dot, 16, 64);          // q . gr
                if (m) {
                    const float nrm = sqrtf(nn);
                    const bool ok = nrm > 1e-12f;
                    const float inv = ok ? 1.0f / nrm : 1e12f;                    // clamped norm: d rot = gr / eps
                    const float dot = ok ? qd * inv * inv : 0.0f;                 // (rhat . gr) / n
                    if (half == 0) {
                        const float* off = d.in.offset + ((size_t)a * k + j) * 3;
#pragma unroll
                        for (int i = 0; i < 3; i++) {
                            const float gx = p.og.xyz[(size_t)row * 3 + i];
                            dA[i] += gx;
                            p.d_offset[((size_t)a * k + j) * 3 + i] = gx * S[i];
                            dS[i] = fmaf(gx, off[i], dS[i]);
                            const float sg = sigmoid_(y[i]);
                            const float gs = p.og.scaling[(size_t)row * 3 + i];
                            g[i] = gs * S[3 + i] * sg * (1.0f - sg);
                            dS[3 + i] = fmaf(gs, sg, dS[3 + i]);
                        }
                        g[3] = (gr.x - y[3] * dot) * inv;
                    } else {
                        g[0] = (gr.y - y[0] * dot) * inv; g[1] = (gr.z - y[1] * dot) * inv; g[2] = (gr.w - y[2] * dot) * inv;
                    }
                }
#pragma unroll
                for (int r = 0; r < 4; r++) {                                     // scratch keeps the ORIGINAL row order 7 j + c
                    const int c = 4 * half + r;
                    if (j < k && c < 7) SC_AT(sc, tile, SC_P2C + 7 * j + c, n) = g[r];
                }
            } else {                         // colour = sigmoid(.); lane kk = offset 4 ot + kk
                const int j = 4 * ot + kk;
                if (j < k && ((mbits >> j) & 1u)) {
                    const uint32_t row = row0 + __popc(mbits & ((1u << j) - 1u));
#pragma unroll
                    for (int r = 0; r < 3; r++) {
                        const float c = sigmoid_(y[r]);
                        g[r] = p.og.color[(size_t)row * 3 + r] * c * (1.0f - c);
                    }
                }
#pragma unroll
                for (int r = 0; r < 3; r++)
                    if (j < k) SC_AT(sc, tile, SC_P2K + 3 * j + r, n) = g[r];
            }
#pragma unroll
            for (int ht = 0; ht < 2; ht++)
#pragma unroll
                for (int r = 0; r < 4; r++) dh[ht] = MFMA(lds[(L_W2T + (ht * NOT + ot) * 4 + r) * 64 + lane], g[r], dh[ht]);
        }
#pragma unroll
        for (int ht = 0; ht < 2; ht++) {
#pragma unroll
            for (int r = 0; r < 4; r++) dh[ht][r] = acc[ht][r] > 0.0f ? dh[ht][r] : 0.0f;
            store_tile(sc, tile, SC_H + 32 * HEAD + 16 * ht, kk, n, hb[ht]);
            store_tile(sc, tile, SC_P1 + 32 * HEAD + 16 * ht, kk, n, dh[ht]);
        }
        if (HEAD == 1) {
#pragma unroll
            for (int i = 0; i < 3; i++) { dA[i] += __shfl_xor(dA[i], 16, 64); dA[i] += __shfl_xor(dA[i], 32, 64); }
#pragma unroll
            for (int i = 0; i < 6; i++) { dS[i] += __shfl_xor(dS[i], 16, 64); dS[i] += __shfl_xor(dS[i], 32, 64); }
            if (kk == 0) {
#pragma unroll
                for (int i = 0; i < 3; i++) SC_AT(sc, tile, SC_GEO + i, n) = dA[i];
#pragma unroll
                for (int i = 0; i < 6; i++) SC_AT(sc, tile, SC_GEO + 3 + i, n) = dS[i];
            }
        }
    }
}

#define BWD_LDS_SLOTS 208     // the cov head: 24 + 64 + 32 + 64 + 24
__global__ void __launch_bounds__(GSD_BLOCK) k_dec_bwd_heads(BwdArgs p)
{
    extern __shared__ float lds[];
    if (blockIdx.y == 0) bwd_head<0>(p, lds);
    else if (blockIdx.y == 1) bwd_head<1>(p, lds);
    else bwd_head<2>(p, lds);
}

// dX^T = [W1o; W1c; W1k]^T dpre1 (96 -> 48 x columns) per 16-anchor tile, then the per-anchor gradients
__global__ void __launch_bounds__(GSD_BLOCK) k_dec_bwd_dx(DecArgs p, const float* __restrict__ img, const float* __restrict__ sc,
                                                         float* __restrict__ d_anchor, float* __restrict__ d_feat, float* __restrict__ d_scaling,
                                                         int n_tiles)
{
    __shared__ float lds[72 * 64];
    img_to_lds(lds, 0, img, IMG_W1T, 72);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, kk = lane >> 4;
    for (int tile = blockIdx.x * (GSD_BLOCK / 64) + wave; tile < n_tiles; tile += gridDim.x * (GSD_BLOCK / 64)) {
        const int v = tile * 16 + n;
        if (tile * 16 >= p.cfg.Nv) continue;
        int a;
        const bool active = row_anchor(p.in.vis_idx, v, p.cfg.Nv, a);
        f32x4 dx[3];
#pragma unroll
        for (int xt = 0; xt < 3; xt++) dx[xt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int h = 0; h < 3; h++)
#pragma unroll
            for (int ht = 0; ht < 2; ht++) {
                f32x4 g;
#pragma unroll
                for (int r = 0; r < 4; r++) g[r] = SC_AT(sc, tile, SC_P1 + 32 * h + 16 * ht + 4 * kk + r, n);
#pragma unroll
                for (int xt = 0; xt < 3; xt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) dx[xt] = MFMA(lds[(((h * 3 + xt) * 2 + ht) * 4 + r) * 64 + lane], g[r], dx[xt]);
            }
        if (active) {
            float4* f4 = reinterpret_cast<float4*>(d_feat + (size_t)a * GSD_FEAT);
            f4[kk] = make_float4(dx[0][0], dx[0][1], dx[0][2], dx[0][3]);
            f4[4 + kk] = make_float4(dx[1][0], dx[1][1], dx[1][2], dx[1][3]);
            if (kk == 0) {       // x columns 32..35 = view, dist
                const float r0 = p.in.anchor[3 * a] - p.in.campos[0], r1 = p.in.anchor[3 * a + 1] - p.in.campos[1],
                            r2 = p.in.anchor[3 * a + 2] - p.in.campos[2];
                const float dist = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
                const float vw[3] = {r0 / dist, r1 / dist, r2 / dist};
                const float vd = vw[0] * dx[2][0] + vw[1] * dx[2][1] + vw[2] * dx[2][2];
#pragma unroll
                for (int i = 0; i < 3; i++)
                    d_anchor[3 * a + i] = SC_AT(sc, tile, SC_GEO + i, n) + (dx[2][i] - vw[i] * vd) / dist + dx[2][3] * vw[i];
#pragma unroll
                for (int i = 0; i < 6; i++) d_scaling[(size_t)a * 6 + i] = SC_AT(sc, tile, SC_GEO + 3 + i, n);
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------ backward, weight gradients (MFMA)
// One problem = one 16-column group of gradient columns (A, rows of dW) against NB 16-column groups of activation columns (B).
struct WgProblem { int a_col; int b_col; int nb; };
struct WgArgs {
    const float* sc; size_t ld; int n_chunks; int n_prob;
    float* part;            // [n_prob][WG_WAVES][3][256] tile partials
    float* bias_part;       // [n_prob][WG_WAVES][16]
    WgProblem prob[WG_MAXPROB];
};
__global__ void __launch_bounds__(64) k_wgrad(WgArgs p)
{
    const WgProblem pr = p.prob[blockIdx.y];
    const int lane = threadIdx.x, i = lane & 15, kk = lane >> 4;
    f32x4 acc[3];
#pragma unroll
    for (int nb = 0; nb < 3; nb++) acc[nb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float bsum = 0.0f;
    // chunk c = anchors 64 c .. 64 c + 63 = tiles 4 c .. 4 c + 3; lane (i, kk) reads the 16 anchors of tile 4 c + kk for its column
    const float* colA = p.sc + ((size_t)kk * SC_COLS + pr.a_col + i) * 16;
    const float* colB = p.sc + ((size_t)kk * SC_COLS + pr.b_col + i) * 16;
    // A wave walks ~4.5 chunks; every chunk's loads (A and up to three B column groups, 16 float4 per lane) go out together -- group by
    // group behind the `nb < pr.nb` test they were four dependent round trips per chunk.  Groups beyond pr.nb re-read group 0 (a valid
    // address) and their products are not formed.
    for (int c = blockIdx.x; c < p.n_chunks; c += gridDim.x) {
        const size_t o = (size_t)c * 4 * SC_COLS * 16;
        float4 a4[4], b4[3][4];
#pragma unroll
        for (int q = 0; q < 4; q++) a4[q] = reinterpret_cast<const float4*>(colA + o)[q];
#pragma unroll
        for (int nb = 0; nb < 3; nb++)
#pragma unroll
            for (int q = 0; q < 4; q++) b4[nb][q] = reinterpret_cast<const float4*>(colB + (size_t)(16 * (nb < pr.nb ? nb : 0)) * 16 + o)[q];
#pragma unroll
        for (int q = 0; q < 4; q++) bsum += (a4[q].x + a4[q].y) + (a4[q].z + a4[q].w);
#pragma unroll
        for (int nb = 0; nb < 3; nb++) {
            if (nb < pr.nb) {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q].x, b4[nb][q].x, acc[nb], 0, 0, 0);
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q].y, b4[nb][q].y, acc[nb], 0, 0, 0);
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q].z, b4[nb][q].z, acc[nb], 0, 0, 0);
                    acc[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a4[q].w, b4[nb][q].w, acc[nb], 0, 0, 0);
                }
            }
        }
    }
    // D layout: lane holds D[m = 4*(lane/16) + r][n = lane%16]
    float* out = p.part + ((size_t)blockIdx.y * WG_WAVES + blockIdx.x) * 3 * 256;
#pragma unroll
    for (int nb = 0; nb < 3; nb++)
#pragma unroll
        for (int r = 0; r < 4; r++) out[nb * 256 + (4 * kk + r) * 16 + i] = acc[nb][r];
    bsum += __shfl_xor(bsum, 16, 64);
    bsum += __shfl_xor(bsum, 32, 64);
    if (kk == 0) p.bias_part[((size_t)blockIdx.y * WG_WAVES + blockIdx.x) * 16 + i] = bsum;
}

// sum the partial tiles over the persistent waves and scatter into the nn.Linear-shaped gradients
struct WgOut {
    gsd_cfg cfg;
    gsd_params g;           // destinations
    const float* part; const float* bias_part; int n_waves; int n_prob;
    // per problem: head (0 o, 1 c, 2 k), layer (1 or 2), first output row of the 16-row group
    int head[WG_MAXPROB], layer[WG_MAXPROB], row0[WG_MAXPROB], nb[WG_MAXPROB];
    // appearance: dW1k[:, app cols] = db1k (x) app;  dapp = W1k[:, app cols]^T db1k  (db1k from the two layer-1 problems of head k)
    const float* W1k; const float* app; int app_prob[2];
};
__global__ void __launch_bounds__(256) k_wgrad_reduce(WgOut p)
{
    const int pi = blockIdx.x, nbsel = blockIdx.y;
    if (pi == p.n_prob) {                               // the appearance block
        __shared__ float db[32];
        if (nbsel != 0 || p.cfg.A == 0) return;
        if (threadIdx.x < 32) {
            const int q = p.app_prob[threadIdx.x >> 4];
            float s = 0.0f;
#pragma unroll 8
            for (int w = 0; w < p.n_waves; w++) s += p.bias_part[((size_t)q * WG_WAVES + w) * 16 + (threadIdx.x & 15)];
            db[threadIdx.x] = s;
        }
        __syncthreads();
        const int A = p.cfg.A, base = 35 + (p.cfg.dist_k ? 1 : 0) + (p.cfg.level ? 1 : 0), in = base + A;
        for (int e = threadIdx.x; e < 32 * A; e += 256) {
            const int j = e / A, i = e % A;
            p.g.W1k[j * in + base + i] = db[j] * p.app[i];
        }
        if (threadIdx.x < A) {
            float s = 0.0f;
            for (int j = 0; j < 32; j++) s = fmaf(p.W1k[j * in + base + threadIdx.x], db[j], s);
            p.g.app[threadIdx.x] = s;
        }
        return;
    }
    if (nbsel > p.nb[pi]) return;                       // nbsel == nb  -> the bias vector
    const int head = p.head[pi], layer = p.layer[pi];
    const int k = p.cfg.k, lv = p.cfg.level ? 1 : 0;
    const int dist = head == 0 ? p.cfg.dist_o : (head == 1 ? p.cfg.dist_c : p.cfg.dist_k);
    const int out_dim = layer == 1 ? 32 : (head == 0 ? k : (head == 1 ? 7 * k : 3 * k));
    const int in1 = 35 + (dist ? 1 : 0) + lv + (head == 2 ? p.cfg.A : 0);
    float* W = layer == 1 ? (head == 0 ? p.g.W1o : head == 1 ? p.g.W1c : p.g.W1k) : (head == 0 ? p.g.W2o : head == 1 ? p.g.W2c : p.g.W2k);
    float* B = layer == 1 ? (head == 0 ? p.g.b1o : head == 1 ? p.g.b1c : p.g.b1k) : (head == 0 ? p.g.b2o : head == 1 ? p.g.b2c : p.g.b2k);
    if (nbsel == p.nb[pi]) {
        if (threadIdx.x < 16) {
            float s = 0.0f;
#pragma unroll 8
            for (int w = 0; w < p.n_waves; w++) s += p.bias_part[((size_t)pi * WG_WAVES + w) * 16 + threadIdx.x];
            const int row = p.row0[pi] + threadIdx.x;
            if (row < out_dim) B[row] = s;
        }
        return;
    }
    const int m = threadIdx.x >> 4, n = threadIdx.x & 15;
    float s = 0.0f;
#pragma unroll 8
    for (int w = 0; w < p.n_waves; w++) s += p.part[(((size_t)pi * WG_WAVES + w) * 3 + nbsel) * 256 + threadIdx.x];
    const int row = p.row0[pi] + m, col = 16 * nbsel + n;
    if (row >= out_dim) return;
    if (layer == 2) { W[row * 32 + col] = s; return; }
    // layer 1: scratch column -> nn.Linear input column
    int dst = -1;
    if (col < 35) dst = col;
    else if (col == 35) dst = dist ? 35 : -1;
    else if (col == 36) dst = lv ? 35 + (dist ? 1 : 0) : -1;
    if (dst >= 0) W[row * in1 + dst] = s;
}

// ------------------------------------------------------------------------------------------------ host side
static int check_cfg(const gsd_cfg* c, const gsd_inputs* in, const gsd_params* p)
{
    if (!c || !in || !p) { gsr_set_error("gsd: null cfg/inputs/params"); return 1; }
    if (c->k < 1 || c->k > GSD_MAX_K) { gsr_set_error("gsd: n_offsets k=%d out of range [1,%d]", c->k, GSD_MAX_K); return 1; }
    if (c->A < 0 || c->A > GSD_MAX_APP) { gsr_set_error("gsd: appearance_dim A=%d out of range [0,%d]", c->A, GSD_MAX_APP); return 1; }
    if (c->Na < 0 || c->Nv < 0 || c->Nv > c->Na) { gsr_set_error("gsd: bad sizes Na=%d Nv=%d", c->Na, c->Nv); return 1; }
    if (c->Nv && (!in->anchor || !in->feat || !in->offset || !in->scaling || !in->vis_idx || !in->campos)) {
        gsr_set_error("gsd: anchor/feat/offset/scaling/vis_idx/campos must be provided"); return 1;
    }
    if (c->level && !in->level) { gsr_set_error("gsd: add_level set but level is NULL"); return 1; }
    if (!p->W1o || !p->b1o || !p->W2o || !p->b2o || !p->W1c || !p->b1c || !p->W2c || !p->b2c || !p->W1k || !p->b1k || !p->W2k || !p->b2k ||
        (c->A && !p->app)) { gsr_set_error("gsd: missing MLP parameter pointer"); return 1; }
    if (((uintptr_t)in->feat | (uintptr_t)p->W2o | (uintptr_t)p->W2c | (uintptr_t)p->W2k) & 15) {
        gsr_set_error("gsd: feat and the layer-2 weights must be 16-byte aligned"); return 1;
    }
    return 0;
}

static DecArgs make_args(const gsd_cfg* c, const gsd_inputs* in)
{
    DecArgs a;
    a.cfg = *c; a.in = *in;
    return a;
}

static void launch_pack(const gsd_cfg* c, const gsd_params* p, float* img, uint32_t* scan_flags, uint32_t n_scan_flags, hipStream_t s)
{
    PackArgs pa;
    pa.scan_flags = scan_flags; pa.n_scan_flags = n_scan_flags;
    pa.cfg = *c;
    pa.W1o = p->W1o; pa.b1o = p->b1o; pa.W2o = p->W2o; pa.b2o = p->b2o;
    pa.W1c = p->W1c; pa.b1c = p->b1c; pa.W2c = p->W2c; pa.b2c = p->b2c;
    pa.W1k = p->W1k; pa.b1k = p->b1k; pa.W2k = p->W2k; pa.b2k = p->b2k;
    pa.app = p->app; pa.img = img;
    hipLaunchKernelGGL(k_pack_img, dim3(gsr_div_up(IMG_FLOATS, 256)), dim3(256), 0, s, pa);
}
static int tile_grid(int n_tiles, int waves_per_block, int max_blocks)
{
    const int b = (n_tiles + waves_per_block - 1) / waves_per_block;
    return b < max_blocks ? (b > 0 ? b : 1) : max_blocks;
}

// forward scratch: [weight image][total word (256 B)][scan block sums]
static size_t fwd_sums_off() { return gsr_align(IMG_FLOATS * sizeof(float)) + 256; }
extern "C" size_t gsd_forward_scratch_bytes(int32_t Nv)
{
    return fwd_sums_off() + gsr_align(((size_t)gsr_div_up((uint32_t)(Nv > 0 ? Nv : 1), 1024u) + 1) * sizeof(uint32_t));
}
extern "C" size_t gsd_compact_scratch_bytes(int32_t Na)
{
    const size_t n = (size_t)(Na > 0 ? Na : 1);
    return 256 + gsr_align(n * sizeof(uint32_t)) + gsr_align(((n + 1023) / 1024 + 1) * sizeof(uint32_t));
}

extern "C" int gsd_compact_visible(const uint8_t* mask, int32_t Na, int32_t* vis_idx, uint32_t* count_host, void* scratch,
                                   size_t scratch_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (!count_host) { gsr_set_error("gsd_compact_visible: count_host is NULL"); return 1; }
    *count_host = 0;
    if (Na <= 0) return 0;
    if (!mask || !vis_idx || !scratch || scratch_bytes < gsd_compact_scratch_bytes(Na)) {
        gsr_set_error("gsd_compact_visible: null pointer or scratch too small"); return 1;
    }
    uint32_t* total = (uint32_t*)scratch;
    uint32_t* pos = (uint32_t*)((char*)scratch + 256);
    uint32_t* sums = (uint32_t*)((char*)pos + gsr_align((size_t)Na * sizeof(uint32_t)));
    hipLaunchKernelGGL(k_flags, dim3(gsr_div_up(Na, 256)), dim3(256), 0, s, mask, (uint32_t)Na, pos, sums, gsr_div_up((uint32_t)Na, 1024u));
    launch_scan(pos, (uint32_t)Na, sums, total, s);
    hipLaunchKernelGGL(k_scatter_idx, dim3(gsr_div_up(Na, 256)), dim3(256), 0, s, mask, (uint32_t)Na, pos, vis_idx);
    GSR_CHECK(hipMemcpyAsync(count_host, total, sizeof(uint32_t), hipMemcpyDeviceToHost, s), "gsd_compact_visible: copy");
    GSR_CHECK(hipStreamSynchronize(s), "gsd_compact_visible: sync");
    if (*count_host == GSD_SCAN_POISON) { *count_host = 0; gsr_set_error("gsd_compact_visible: %s", GSD_SCAN_TIMEOUT_MSG); return 1; }
    return gsr_check_launch("gsd_compact_visible", s, false);
}

// The same compaction WITHOUT the host synchronisation: vis_idx gets all Na entries, the visible anchors' indices first (ascending) and -1
// behind them; the caller runs the decode with Nv = Na and the kernels skip the padding rows.  *count_dev (device, may be NULL) receives
// the number of visible anchors -- or 0xFFFFFFFF when the scan's bounded look-back timed out (no host is in the loop to raise: vis_idx then holds
// in-range indices and -1 only, and a caller that later reads the count sees the poison).
extern "C" int gsd_compact_visible_padded(const uint8_t* mask, int32_t Na, int32_t* vis_idx, uint32_t* count_dev, void* scratch,
                                          size_t scratch_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (Na <= 0) return 0;
    if (!mask || !vis_idx || !scratch || scratch_bytes < gsd_compact_scratch_bytes(Na)) {
        gsr_set_error("gsd_compact_visible_padded: null pointer or scratch too small"); return 1;
    }
    uint32_t* total = (uint32_t*)scratch;
    uint32_t* pos = (uint32_t*)((char*)scratch + 256);
    uint32_t* sums = (uint32_t*)((char*)pos + gsr_align((size_t)Na * sizeof(uint32_t)));
    if (gsr_memset_async(vis_idx, 0xFF, (size_t)Na * sizeof(int32_t), s)) { gsr_set_error("gsd_compact_visible_padded: fill"); return 1; };
    hipLaunchKernelGGL(k_flags, dim3(gsr_div_up(Na, 256)), dim3(256), 0, s, mask, (uint32_t)Na, pos, sums, gsr_div_up((uint32_t)Na, 1024u));
    launch_scan(pos, (uint32_t)Na, sums, total, s);
    hipLaunchKernelGGL(k_scatter_idx, dim3(gsr_div_up(Na, 256)), dim3(256), 0, s, mask, (uint32_t)Na, pos, vis_idx);
    if (count_dev) GSR_CHECK(hipMemcpyAsync(count_dev, total, sizeof(uint32_t), hipMemcpyDeviceToDevice, s), "gsd_compact_visible_padded: count");
    return gsr_check_launch("gsd_compact_visible_padded", s, false);
}

static int fwd_checks(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, void* scratch, size_t scratch_bytes, const char* who)
{
    if (check_cfg(cfg, in, p)) return 1;
    if (!scratch || scratch_bytes < gsd_forward_scratch_bytes(cfg->Nv)) { gsr_set_error("%s: scratch too small", who); return 1; }
    return 0;
}
static uint32_t* fwd_total(void* scratch) { return (uint32_t*)((char*)scratch + gsr_align(IMG_FLOATS * sizeof(float))); }

// image + opacity head + scan: row_offset final, device total in fwd_total(scratch)[0]
static void enqueue_stage1(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, float* neural_opacity, uint8_t* mask,
                           uint32_t* row_offset, void* scratch, hipStream_t s)
{
    float* img = (float*)scratch;
    uint32_t* total = fwd_total(scratch);
    uint32_t* sums = (uint32_t*)((char*)scratch + fwd_sums_off());
    const uint32_t nblk = gsr_div_up((uint32_t)(cfg->Nv > 0 ? cfg->Nv : 1), 1024u);
    launch_pack(cfg, p, img, sums, nblk, s);
    if (cfg->Nv == 0) return;
    DecArgs a = make_args(cfg, in);
    const int n_tiles = (cfg->Nv + 15) / 16;
    hipLaunchKernelGGL(k_dec_opacity, dim3(tile_grid(n_tiles, GSD_BLOCK / 64, 2048)), dim3(GSD_BLOCK), 0, s, a, (const float*)img,
                       neural_opacity, mask, row_offset, n_tiles);
    hipLaunchKernelGGL(k_scan_lookback, dim3(nblk), dim3(1024), 0, s, row_offset, (uint32_t)cfg->Nv, sums, total);
}
static void enqueue_stage2(const gsd_cfg* cfg, const gsd_inputs* in, const float* neural_opacity, const uint32_t* row_offset,
                           const gsd_outputs* out, const void* scratch, hipStream_t s)
{
    DecArgs a = make_args(cfg, in);
    const int n_tiles = (cfg->Nv + 15) / 16;
    hipLaunchKernelGGL(k_dec_emit, dim3(tile_grid(n_tiles, GSD_BLOCK / 64, 1024), 2), dim3(GSD_BLOCK), 0, s, a, (const float*)scratch,
                       neural_opacity, row_offset, *out, n_tiles);
}
static int check_outputs(const gsd_outputs* out, const char* who)
{
    if (!out || !out->xyz || !out->color || !out->opacity || !out->scaling || !out->rot) { gsr_set_error("%s: null output", who); return 1; }
    if ((uintptr_t)out->rot & 15) { gsr_set_error("%s: rot must be 16-byte aligned", who); return 1; }
    return 0;
}

extern "C" int gsd_forward_stage1(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, float* neural_opacity, uint8_t* mask,
                                  uint32_t* row_offset, uint32_t* P_host, void* scratch, size_t scratch_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (fwd_checks(cfg, in, p, scratch, scratch_bytes, "gsd_forward_stage1")) return 1;
    if (!P_host) { gsr_set_error("gsd_forward_stage1: P_host is NULL"); return 1; }
    *P_host = 0;
    if (cfg->Nv && (!neural_opacity || !mask || !row_offset)) { gsr_set_error("gsd_forward_stage1: null output"); return 1; }
    enqueue_stage1(cfg, in, p, neural_opacity, mask, row_offset, scratch, s);
    if (cfg->Nv == 0) return gsr_check_launch("gsd_forward_stage1", s, false);
    GSR_CHECK(hipMemcpyAsync(P_host, fwd_total(scratch), sizeof(uint32_t), hipMemcpyDeviceToHost, s), "gsd_forward_stage1: copy");
    GSR_CHECK(hipStreamSynchronize(s), "gsd_forward_stage1: sync");
    if (*P_host == GSD_SCAN_POISON) { *P_host = 0; gsr_set_error("gsd_forward_stage1: %s", GSD_SCAN_TIMEOUT_MSG); return 1; }
    return gsr_check_launch("gsd_forward_stage1", s, false);
}

extern "C" int gsd_forward_stage2(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, const float* neural_opacity,
                                  const uint32_t* row_offset, uint32_t P, const gsd_outputs* out, void* scratch, size_t scratch_bytes,
                                  void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (fwd_checks(cfg, in, p, scratch, scratch_bytes, "gsd_forward_stage2")) return 1;
    if (cfg->Nv == 0 || P == 0) return 0;
    if (check_outputs(out, "gsd_forward_stage2")) return 1;
    if (!neural_opacity || !row_offset) { gsr_set_error("gsd_forward_stage2: null input"); return 1; }
    enqueue_stage2(cfg, in, neural_opacity, row_offset, out, scratch, s);      // the weight image was written by stage 1 into `scratch`
    return gsr_check_launch("gsd_forward_stage2", s, false);
}

extern "C" int gsd_forward(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, float* neural_opacity, uint8_t* mask,
                           uint32_t* row_offset, const gsd_outputs* out, uint32_t* P_host, void* scratch, size_t scratch_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (fwd_checks(cfg, in, p, scratch, scratch_bytes, "gsd_forward")) return 1;
    if (!P_host) { gsr_set_error("gsd_forward: P_host is NULL"); return 1; }
    *P_host = 0;
    if (cfg->Nv && (!neural_opacity || !mask || !row_offset)) { gsr_set_error("gsd_forward: null output"); return 1; }
    if (cfg->Nv && check_outputs(out, "gsd_forward")) return 1;
    enqueue_stage1(cfg, in, p, neural_opacity, mask, row_offset, scratch, s);
    if (cfg->Nv == 0) return gsr_check_launch("gsd_forward", s, false);
    enqueue_stage2(cfg, in, neural_opacity, row_offset, out, scratch, s);       // outputs sized for the worst case: no host round trip
    GSR_CHECK(hipMemcpyAsync(P_host, fwd_total(scratch), sizeof(uint32_t), hipMemcpyDeviceToHost, s), "gsd_forward: copy");
    GSR_CHECK(hipStreamSynchronize(s), "gsd_forward: sync");
    if (*P_host == GSD_SCAN_POISON) { *P_host = 0; gsr_set_error("gsd_forward: %s", GSD_SCAN_TIMEOUT_MSG); return 1; }
    return gsr_check_launch("gsd_forward", s, false);
}

// Static-shape forward (round 3): no host synchronisation, so the call can be recorded into a HIP graph and replayed.  The outputs keep their
// worst-case Nv*k rows; the rows behind the P emitted ones are PARKED at the camera centre with zero opacity, so that any rasterizer of this
// library culls them in its preprocess (view depth 0 <= 0.2; radii 0, no tile instance, zero gradients) -- the caller passes all Nv*k rows on
// and never learns P on the host.  *count_dev (DEVICE, optional) <- P, or 0xFFFFFFFF when the scan's bounded look-back timed out: ALL rows are parked then.
__global__ void __launch_bounds__(256) k_park_tail(const uint32_t* __restrict__ total, uint32_t cap, const float* __restrict__ campos,
                                                   float* __restrict__ xyz, float* __restrict__ color, float* __restrict__ opacity,
                                                   float* __restrict__ scaling, float* __restrict__ rot, uint32_t* __restrict__ count_dev)
{
    uint32_t P = *total;
    if (count_dev && blockIdx.x == 0 && threadIdx.x == 0) *count_dev = P;      // GSD_SCAN_POISON (0xFFFFFFFF) when the scan timed out: then ...
    if (P == GSD_SCAN_POISON) P = 0u;                                           // ... EVERY row is parked -- inert outputs, never rows at garbage offsets
    const float cx = campos[0], cy = campos[1], cz = campos[2];
    for (uint32_t i = P + blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += gridDim.x * blockDim.x) {
        xyz[3 * i] = cx; xyz[3 * i + 1] = cy; xyz[3 * i + 2] = cz;
        color[3 * i] = 0.f; color[3 * i + 1] = 0.f; color[3 * i + 2] = 0.f;
        opacity[i] = 0.f;
        scaling[3 * i] = 0.f; scaling[3 * i + 1] = 0.f; scaling[3 * i + 2] = 0.f;
        rot[4 * i] = 1.f; rot[4 * i + 1] = 0.f; rot[4 * i + 2] = 0.f; rot[4 * i + 3] = 0.f;
    }
}
extern "C" int gsd_forward_static(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, float* neural_opacity, uint8_t* mask,
                                  uint32_t* row_offset, const gsd_outputs* out, uint32_t* count_dev, void* scratch, size_t scratch_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (fwd_checks(cfg, in, p, scratch, scratch_bytes, "gsd_forward_static")) return 1;
    if (cfg->Nv && (!neural_opacity || !mask || !row_offset)) { gsr_set_error("gsd_forward_static: null output"); return 1; }
    if (cfg->Nv && check_outputs(out, "gsd_forward_static")) return 1;
    enqueue_stage1(cfg, in, p, neural_opacity, mask, row_offset, scratch, s);
    if (cfg->Nv == 0) { if (count_dev) if (gsr_memset_async(count_dev, 0, sizeof(uint32_t), s)) { gsr_set_error("count"); return 1; }; return gsr_check_launch("gsd_forward_static", s, false); }
    enqueue_stage2(cfg, in, neural_opacity, row_offset, out, scratch, s);
    const uint32_t cap = (uint32_t)cfg->Nv * (uint32_t)cfg->k;
    hipLaunchKernelGGL(k_park_tail, dim3(gsr_div_up(cap, 256u * 8u) + 1u), dim3(256), 0, s, fwd_total(scratch), cap, in->campos, out->xyz, out->color,
                       out->opacity, out->scaling, out->rot, count_dev);
    return gsr_check_launch("gsd_forward_static", s, false);
}

extern "C" int gsd_forward_deferred(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, float* neural_opacity, uint8_t* mask,
                                    uint32_t* row_offset, const gsd_outputs* out, uint32_t* count_host, void* event, void* scratch, size_t scratch_bytes,
                                    void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (fwd_checks(cfg, in, p, scratch, scratch_bytes, "gsd_forward_deferred")) return 1;
    if (!count_host || !event) { gsr_set_error("gsd_forward_deferred: count_host / event is NULL"); return 1; }
    if (cfg->Nv && (!neural_opacity || !mask || !row_offset)) { gsr_set_error("gsd_forward_deferred: null output"); return 1; }
    if (cfg->Nv && check_outputs(out, "gsd_forward_deferred")) return 1;
    enqueue_stage1(cfg, in, p, neural_opacity, mask, row_offset, scratch, s);
    if (cfg->Nv == 0) {
        *count_host = 0u;
        GSR_CHECK(hipEventRecord((hipEvent_t)event, s), "gsd_forward_deferred: event");
        return gsr_check_launch("gsd_forward_deferred", s, false);
    }
    GSR_CHECK(hipMemcpyAsync(count_host, fwd_total(scratch), sizeof(uint32_t), hipMemcpyDeviceToHost, s), "gsd_forward_deferred: count copy");
    GSR_CHECK(hipEventRecord((hipEvent_t)event, s), "gsd_forward_deferred: event");
    enqueue_stage2(cfg, in, neural_opacity, row_offset, out, scratch, s);
    return gsr_check_launch("gsd_forward_deferred", s, false);
}

// backward scratch: [weight image][feature-major columns SC_COLS x ld][tile partials][bias partials]
static size_t bwd_ld(const gsd_cfg* c) { return (size_t)gsr_div_up((uint32_t)(c->Nv > 0 ? c->Nv : 1), GSD_BLOCK) * GSD_BLOCK; }
extern "C" size_t gsd_backward_scratch_bytes(const gsd_cfg* cfg)
{
    if (!cfg) return 0;
    return gsr_align(IMG_FLOATS * sizeof(float)) + gsr_align((size_t)SC_COLS * bwd_ld(cfg) * sizeof(float)) +
           gsr_align((size_t)WG_MAXPROB * WG_WAVES * 3 * 256 * sizeof(float)) + gsr_align((size_t)WG_MAXPROB * WG_WAVES * 16 * sizeof(float));
}

extern "C" int gsd_backward(const gsd_cfg* cfg, const gsd_inputs* in, const gsd_params* p, const float* neural_opacity,
                            const uint32_t* row_offset, uint32_t P, const gsd_out_grads* og, const gsd_in_grads* ig,
                            const void* fwd_scratch, void* scratch, size_t scratch_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    if (check_cfg(cfg, in, p)) return 1;
    if (!ig) { gsr_set_error("gsd_backward: null in_grads"); return 1; }
    const gsd_params& g = ig->params;
    if (!g.W1o || !g.b1o || !g.W2o || !g.b2o || !g.W1c || !g.b1c || !g.W2c || !g.b2c || !g.W1k || !g.b1k || !g.W2k || !g.b2k || (cfg->A && !g.app)) {
        gsr_set_error("gsd_backward: missing parameter-gradient pointer"); return 1;
    }
    if (!scratch || scratch_bytes < gsd_backward_scratch_bytes(cfg)) { gsr_set_error("gsd_backward: scratch too small"); return 1; }
    const int k = cfg->k;
    if (cfg->Nv == 0 || P == 0) {       // no anchors, or every gate closed (no output row, the out-gradient tensors are empty): all parameter gradients are zero;
                                        // the per-anchor gradients are the caller's zero-filled buffers
        const int lv = cfg->level ? 1 : 0;
        (void)gsr_memset_async(g.W1o, 0, sizeof(float) * 32 * (35 + (cfg->dist_o ? 1 : 0) + lv), s); (void)gsr_memset_async(g.b1o, 0, sizeof(float) * 32, s);
        (void)gsr_memset_async(g.W1c, 0, sizeof(float) * 32 * (35 + (cfg->dist_c ? 1 : 0) + lv), s); (void)gsr_memset_async(g.b1c, 0, sizeof(float) * 32, s);
        (void)gsr_memset_async(g.W1k, 0, sizeof(float) * 32 * (35 + (cfg->dist_k ? 1 : 0) + lv + cfg->A), s); (void)gsr_memset_async(g.b1k, 0, sizeof(float) * 32, s);
        (void)gsr_memset_async(g.W2o, 0, sizeof(float) * 32 * k, s); (void)gsr_memset_async(g.b2o, 0, sizeof(float) * k, s);
        (void)gsr_memset_async(g.W2c, 0, sizeof(float) * 32 * 7 * k, s); (void)gsr_memset_async(g.b2c, 0, sizeof(float) * 7 * k, s);
        (void)gsr_memset_async(g.W2k, 0, sizeof(float) * 32 * 3 * k, s); (void)gsr_memset_async(g.b2k, 0, sizeof(float) * 3 * k, s);
        if (cfg->A) (void)gsr_memset_async(g.app, 0, sizeof(float) * cfg->A, s);
        return gsr_check_launch("gsd_backward", s, false);
    }
    if (!og || !og->xyz || !og->color || !og->opacity || !og->scaling || !og->rot || !ig->anchor || !ig->feat || !ig->offset || !ig->scaling ||
        !neural_opacity || !row_offset) { gsr_set_error("gsd_backward: null gradient pointer"); return 1; }
    if (((uintptr_t)og->rot | (uintptr_t)ig->feat) & 15) { gsr_set_error("gsd_backward: dL_drot / d_feat must be 16-byte aligned"); return 1; }
    const size_t ld = bwd_ld(cfg);
    const float* img = fwd_scratch ? (const float*)fwd_scratch : (const float*)scratch;
    float* sc = (float*)((char*)scratch + gsr_align(IMG_FLOATS * sizeof(float)));
    float* part = (float*)((char*)sc + gsr_align((size_t)SC_COLS * ld * sizeof(float)));
    float* bias_part = (float*)((char*)part + gsr_align((size_t)WG_MAXPROB * WG_WAVES * 3 * 256 * sizeof(float)));
    if (!fwd_scratch) launch_pack(cfg, p, (float*)scratch, nullptr, 0u, s);
    DecArgs a = make_args(cfg, in);
    {
        const int n_tiles = (int)(ld / 16);
        BwdArgs ba;
        ba.d = a; ba.img = img; ba.neural_opacity = neural_opacity; ba.row_offset = row_offset; ba.og = *og; ba.d_offset = ig->offset;
        ba.sc = sc; ba.n_tiles = n_tiles;
        hipLaunchKernelGGL(k_dec_bwd_heads, dim3(tile_grid(n_tiles, GSD_BLOCK / 64, 512), 3), dim3(GSD_BLOCK),
                           (size_t)BWD_LDS_SLOTS * 64 * sizeof(float), s, ba);
        hipLaunchKernelGGL(k_dec_bwd_dx, dim3(tile_grid(n_tiles, GSD_BLOCK / 64, 1024)), dim3(GSD_BLOCK), 0, s, a, img,
                           (const float*)sc, ig->anchor, ig->feat, ig->scaling, n_tiles);
    }

    // weight-gradient problems
    WgArgs wa; WgOut wo;
    wa.sc = sc; wa.ld = ld; wa.n_chunks = (int)(ld / 64); wa.part = part; wa.bias_part = bias_part;
    wo.cfg = *cfg; wo.g = g; wo.part = part; wo.bias_part = bias_part;
    int np = 0;
    wo.W1k = p->W1k; wo.app = p->app; wo.app_prob[0] = wo.app_prob[1] = 0;
    auto add = [&](int a_col, int b_col, int nb, int head, int layer, int row0) {
        if (head == 2 && layer == 1) wo.app_prob[row0 / 16] = np;
        wa.prob[np] = {a_col, b_col, nb}; wo.head[np] = head; wo.layer[np] = layer; wo.row0[np] = row0; wo.nb[np] = nb; np++;
    };
    const int p2col[3] = {SC_P2O, SC_P2C, SC_P2K};
    const int outd[3] = {k, 7 * k, 3 * k};
    for (int head = 0; head < 3; head++) {
        for (int r0 = 0; r0 < outd[head]; r0 += 16) add(p2col[head] + r0, SC_H + 32 * head, 2, head, 2, r0);
        for (int r0 = 0; r0 < 32; r0 += 16) add(SC_P1 + 32 * head + r0, SC_X, 3, head, 1, r0);
    }
    wa.n_prob = np; wo.n_prob = np;
    const int waves = wa.n_chunks < WG_WAVES ? wa.n_chunks : WG_WAVES;
    wo.n_waves = waves;
    hipLaunchKernelGGL(k_wgrad, dim3(waves, np), dim3(64), 0, s, wa);
    hipLaunchKernelGGL(k_wgrad_reduce, dim3(np + 1, 4), dim3(256), 0, s, wo);
    return gsr_check_launch("gsd_backward", s, false);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Per-iteration densification statistics (gssr/gaussian/scaffold_gaussian.py:488-508 training_statis; Octree-GS calls the same method).
// The reference maps generated Gaussians back to (anchor, offset) slots with three boolean-mask assignments and two masked gathers -- six
// nonzero() host synchronisations per iteration.  Here the slot -> Gaussian map is the exclusive prefix of the opacity gate, rebuilt by a
// 3-kernel anchor-level scan (count, scan of block sums, apply): no synchronisation, ~15 us.
#define ST_BLOCK 256
__device__ __forceinline__ uint32_t st_count(const uint8_t* __restrict__ mask, int v, int k)
{
    uint32_t c = 0;
    for (int j = 0; j < k; ++j) c += mask[(size_t)v * k + j] ? 1u : 0u;
    return c;
}

__global__ void __launch_bounds__(ST_BLOCK) k_stats_count(int Nv, int k, const uint8_t* __restrict__ mask, uint32_t* __restrict__ blocksum)
{
    __shared__ uint32_t ws[ST_BLOCK / 64];
    const int v = blockIdx.x * ST_BLOCK + threadIdx.x;
    const uint32_t c = wave_sum(v < Nv ? st_count(mask, v, k) : 0u);
    if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) blocksum[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

__global__ void __launch_bounds__(ST_BLOCK) k_stats_apply(int Nv, int k, const int32_t* __restrict__ vis_idx, const float* __restrict__ nop,
                                                          const uint8_t* __restrict__ mask, const uint8_t* __restrict__ upd, const float* __restrict__ grad,
                                                          int gs, const uint32_t* __restrict__ blockoff, float* __restrict__ opacity_accum,
                                                          float* __restrict__ anchor_demon, float* __restrict__ off_grad, float* __restrict__ off_den)
{
    __shared__ uint32_t lds[17];
    const int v = blockIdx.x * ST_BLOCK + threadIdx.x;
    uint32_t all;
    uint32_t p = blockoff[blockIdx.x] + block_excl_scan(v < Nv ? st_count(mask, v, k) : 0u, lds, &all);
    if (v >= Nv) return;
    const int a = vis_idx[v];
    if (a < 0) return;                                                // padding row (gsd_compact_visible_padded)
    float s = 0.f;
    for (int j = 0; j < k; ++j) { const float o = nop[(size_t)v * k + j]; s += o < 0.f ? 0.f : o; }
    opacity_accum[a] += s; anchor_demon[a] += 1.f;                    // one thread per visible anchor, anchors distinct: plain read-modify-write
    for (int j = 0; j < k; ++j) {
        if (!mask[(size_t)v * k + j]) continue;
        if (upd[p]) {
            const float gx = grad[(size_t)p * gs], gy = grad[(size_t)p * gs + 1];
            off_grad[(size_t)a * k + j] += sqrtf(gx * gx + gy * gy);
            off_den[(size_t)a * k + j] += 1.f;
        }
        ++p;
    }
}

extern "C" size_t gsd_training_stats_scratch_bytes(int32_t Nv) { return gsr_align(((size_t)(Nv > 0 ? Nv : 1) + ST_BLOCK - 1) / ST_BLOCK * sizeof(uint32_t)); }

extern "C" int gsd_training_stats(int32_t Nv, int32_t k, const int32_t* vis_idx, const float* neural_opacity, const uint8_t* mask,
                                  const uint8_t* update_filter, const float* viewspace_grad, int32_t grad_stride, float* opacity_accum,
                                  float* anchor_demon, float* offset_gradient_accum, float* offset_denom, void* scratch, size_t scratch_bytes,
                                  void* stream)
{
    if (Nv <= 0) return 0;
    if (k <= 0 || grad_stride < 2) { gsr_set_error("training_stats: bad sizes k=%d grad_stride=%d", k, grad_stride); return 1; }
    if (!vis_idx || !neural_opacity || !mask || !update_filter || !viewspace_grad || !opacity_accum || !anchor_demon || !offset_gradient_accum ||
        !offset_denom || !scratch || scratch_bytes < gsd_training_stats_scratch_bytes(Nv)) {
        gsr_set_error("training_stats: null pointer or scratch too small"); return 1;
    }
    hipStream_t s = (hipStream_t)stream;
    const uint32_t nblk = ((uint32_t)Nv + ST_BLOCK - 1) / ST_BLOCK;
    uint32_t* bs = (uint32_t*)scratch;
    hipLaunchKernelGGL(k_stats_count, dim3(nblk), dim3(ST_BLOCK), 0, s, Nv, k, mask, bs);
    gsr_scan_small(bs, nblk, 1, 0, nullptr, nullptr, s);
    hipLaunchKernelGGL(k_stats_apply, dim3(nblk), dim3(ST_BLOCK), 0, s, Nv, k, vis_idx, neural_opacity, mask, update_filter, viewspace_grad,
                       grad_stride, (const uint32_t*)bs, opacity_accum, anchor_demon, offset_gradient_accum, offset_denom);
    return gsr_check_launch("training_stats", s, false);
}
