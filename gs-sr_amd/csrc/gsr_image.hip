// gsr_image.hip -- image preparation (include/gsrast.h, "image preparation"): Pillow's 8-bit bicubic resize and the tensors a camera holds.
//   k_img_coeffs   one thread per output coordinate of either axis: (xmin, n) and the int32 taps, float64 and rounded operation by operation
//   k_img_hpass    a workgroup = IM_HSTRIP output columns of one intermediate row; the input bytes the strip needs staged in LDS by aligned dword
//                  loads (ragged head and tail by bytes), premultiplied while staged; one lane = one output pixel, all channels; the taps read LDS.
//                  The span is walked in chunks of IM_STAGE pixels, so any number of taps is exact; the usual 3-4x downscale is one chunk.
//                  It writes a PLANAR intermediate [C][rows][pitch], pitch a multiple of 128: whole dwords, whole lines.
//   k_img_vpass    one wave = IM_VSTRIP output columns of one output row; a lane owns four consecutive bytes of every plane's row (dword loads,
//                  4 C accumulators), the coefficient row is uniform.  Epilogue: un-premultiply, then the uint8 HWC image (through LDS: aligned
//                  dwords, ragged ends by bytes) and the float planes, gray and mask (through LDS: a store instruction covers 256 contiguous bytes).
// Built without FMA contraction (Makefile): the coefficient table and the gray value are products and sums rounded one by one.
#include "gsr_common.h"

#define IM_HSTRIP GSR_IMG_HSTRIP
#define IM_VSTRIP GSR_IMG_VSTRIP
#define IM_VLANES (IM_VSTRIP / 4)
#define IM_STAGE 4096                 // pixels of one staged chunk of the horizontal pass
#define IM_COEFF_BLOCK 64
#define IM_ONE (1 << 22)              // Pillow's PRECISION_BITS = 32 - 8 - 2
#define IM_HALF (1u << 21)
static_assert(IM_VLANES == GSR_WAVE, "the vertical pass is one wave per workgroup");

// One axis as the kernels see it.  K: taps kept per output coordinate (n <= min(ksize, in)).
struct ImAxis { int in, out, identity; double scale, support, ss; int64_t K; };

static ImAxis im_axis(int in, int out)
{
    ImAxis a;
    a.in = in; a.out = out; a.identity = in == out;
    a.scale = (double)in / (double)out;
    const double fs = a.scale < 1.0 ? 1.0 : a.scale;
    a.support = 2.0 * fs;
    a.ss = 1.0 / fs;
    const double ksize = ceil(a.support) * 2.0 + 1.0;
    a.K = a.identity ? 1 : (int64_t)(ksize < (double)in ? ksize : (double)in);
    return a;
}

// (xmin, n) of output coordinate xx; the casts are guarded so that nothing leaves int on the way (the guards change no value inside the range)
static inline __host__ __device__ void im_bounds(const ImAxis& a, int xx, int* xmin, int* n, double* center)
{
    if (a.identity) { *xmin = xx; *n = 1; *center = 0.0; return; }
    const double c = ((double)xx + 0.5) * a.scale;
    const double lo = c - a.support + 0.5, hi = c + a.support + 0.5;
    const int x0 = lo <= 0.0 ? 0 : (int)lo;
    const int x1 = hi >= (double)a.in ? a.in : (int)hi;
    *xmin = x0; *n = x1 - x0; *center = c;
}

static inline __device__ double im_bicubic(double t)
{
    t = fabs(t);
    if (t < 1.0) return ((1.5 * t - 2.5) * t) * t + 1.0;
    if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * -0.5;
    return 0.0;
}

// blocks [0, bx): the horizontal axis, taps TRANSPOSED kk[x * out + xx] (lanes of the pass read neighbours); the rest: the vertical axis, kk[yy * K + x]
__global__ __launch_bounds__(IM_COEFF_BLOCK) void k_img_coeffs(ImAxis ax, ImAxis ay, uint32_t bx, int2* bounds_x, int32_t* kk_x, int2* bounds_y, int32_t* kk_y)
{
    const bool horizontal = blockIdx.x < bx;
    const ImAxis a = horizontal ? ax : ay;
    const int xx = (int)((horizontal ? blockIdx.x : blockIdx.x - bx) * IM_COEFF_BLOCK + threadIdx.x);
    if (xx >= a.out) return;
    int2* bounds = horizontal ? bounds_x : bounds_y;
    int32_t* kk = horizontal ? kk_x + xx : kk_y + (int64_t)xx * a.K;
    const int64_t step = horizontal ? (int64_t)a.out : 1;
    int xmin, n; double center;
    im_bounds(a, xx, &xmin, &n, &center);
    bounds[xx] = make_int2(xmin, n);
    if (a.identity) { kk[0] = IM_ONE; return; }
    double ww = 0.0;
    for (int x = 0; x < n; x++) ww += im_bicubic((((double)(x + xmin) - center) + 0.5) * a.ss);
    for (int x = 0; x < n; x++) {
        double w = im_bicubic((((double)(x + xmin) - center) + 0.5) * a.ss);      // the same operations give the same bits: no table of doubles
        if (ww != 0.0) w = w / ww;
        kk[(int64_t)x * step] = w < 0.0 ? (int)(w * 4194304.0 - 0.5) : (int)(w * 4194304.0 + 0.5);
    }
}

static inline __device__ uint32_t im_clip8(uint32_t acc)
{
    const int v = (int)acc >> 22;
    return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
static inline __device__ uint32_t im_muldiv255(uint32_t c, uint32_t a)
{
    const uint32_t t = c * a + 128u;
    return ((t >> 8) + t) >> 8;
}
static inline __device__ uint32_t im_premultiply(uint32_t px)
{
    const uint32_t a = px >> 24;
    return im_muldiv255(px & 255u, a) | (im_muldiv255((px >> 8) & 255u, a) << 8) | (im_muldiv255((px >> 16) & 255u, a) << 16) | (a << 24);
}

// grid: rows * strips workgroups, row-major.  mid: plane c at mid + c * plane, row r of it at + r * pitch.
template <int C>
__global__ __launch_bounds__(IM_HSTRIP) void k_img_hpass(const uint8_t* __restrict__ img, int64_t stride, int row0, int W, uint32_t strips, int premul,
                                                          const int2* __restrict__ bounds, const int32_t* __restrict__ kk, uint8_t* __restrict__ mid, int64_t plane,
                                                          int pitch)
{
    __shared__ uint32_t stage[IM_STAGE * C / 4 + 2];
    __shared__ uint32_t outb[C][IM_HSTRIP / 4];
    const int tid = (int)threadIdx.x;
    const uint32_t r = blockIdx.x / strips;
    const int x0 = (int)(blockIdx.x % strips) * IM_HSTRIP, xx = x0 + tid, xl = min(x0 + IM_HSTRIP, W) - 1;
    int xmin = 0, n = 0;
    if (xx < W) { const int2 b = bounds[xx]; xmin = b.x; n = b.y; }
    const int2 bf = bounds[x0], bl = bounds[xl];
    const int first = bf.x, last = bl.x + bl.y;           // xmin and xmax do not decrease with xx: the strip reads [first, last)
    const uint8_t* row = img + (int64_t)(row0 + (int)r) * stride;
    uint32_t acc[C];
#pragma unroll
    for (int c = 0; c < C; c++) acc[c] = IM_HALF;
    for (int p0 = first; p0 < last; p0 += IM_STAGE) {
        const int p1 = min(p0 + IM_STAGE, last);
        const uintptr_t g0 = (uintptr_t)(row + (int64_t)p0 * C), g1 = (uintptr_t)(row + (int64_t)p1 * C), a0 = g0 & ~(uintptr_t)3;
        const int head = (int)(g0 - a0), nd = (int)((g1 - a0 + 3) >> 2);      // nd <= IM_STAGE * C / 4 + 2
        if (p0 != first) __syncthreads();                 // the readers of the chunk before
        for (int d = tid; d < nd; d += IM_HSTRIP) {
            const uintptr_t a = a0 + 4u * (uintptr_t)d;
            uint32_t v = 0u;
            if (a >= g0 && a + 4 <= g1) v = *(const uint32_t*)a;
            else                                          // the ragged head or tail: only bytes of this row's span are touched
                for (int j = 0; j < 4; j++) if (a + j >= g0 && a + j < g1) v |= (uint32_t)*(const uint8_t*)(a + j) << (8 * j);
            if (C == 4 && premul) v = im_premultiply(v);  // C == 4: head == 0 and a dword is a pixel (the entry point checks the alignment)
            stage[d] = v;
        }
        __syncthreads();
        const int t0 = max(xmin, p0), t1 = min(xmin + n, p1);
        const int32_t* k = kk + (int64_t)(t0 - xmin) * W + xx;
        if (C == 4) {
            for (int t = t0; t < t1; t++, k += W) {
                const uint32_t kv = (uint32_t)*k, v = stage[t - p0];
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] += kv * ((v >> (8 * c)) & 255u);
            }
        } else {
            const uint8_t* sb = (const uint8_t*)stage + head + (t0 - p0) * C;
            for (int t = t0; t < t1; t++, k += W, sb += C) {
                const uint32_t kv = (uint32_t)*k;
#pragma unroll
                for (int c = 0; c < C; c++) acc[c] += kv * (uint32_t)sb[c];
            }
        }
    }
#pragma unroll
    for (int c = 0; c < C; c++) ((uint8_t*)outb[c])[tid] = (uint8_t)(xx < W ? im_clip8(acc[c]) : 0u);
    __syncthreads();
    const int c = tid / (IM_HSTRIP / 4), d = tid % (IM_HSTRIP / 4);
    if (c < C && x0 + 4 * d < pitch) *(uint32_t*)(mid + (int64_t)c * plane + (int64_t)r * pitch + x0 + 4 * d) = outb[c][d];
}

struct ImOut { uint8_t* u8; float* planes; float* gray; float* mask; int n_planes, unpremul; };

// grid: H * strips workgroups of one wave, row-major
template <int C>
__global__ __launch_bounds__(IM_VLANES) void k_img_vpass(const uint8_t* __restrict__ mid, int64_t plane, int pitch, int row0, int W, int H, uint32_t strips,
                                                          const int2* __restrict__ bounds, const int32_t* __restrict__ kk, int64_t K, ImOut o)
{
    __shared__ uint32_t ob[IM_VSTRIP * C / 4 + 2];
    __shared__ float fb[5][IM_VSTRIP];
    const int lane = (int)threadIdx.x;
    const int y = (int)(blockIdx.x / strips), x0 = (int)(blockIdx.x % strips) * IM_VSTRIP, x = x0 + 4 * lane;
    const int2 b = bounds[y];
    const int32_t* k = kk + (int64_t)y * K;
    uint32_t acc[C][4];
#pragma unroll
    for (int c = 0; c < C; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[c][j] = IM_HALF;
    if (x < pitch) {                                      // pitch is a multiple of 128 and the strip of 256: the last strip may reach past it
        const uint8_t* p = mid + (int64_t)(b.x - row0) * pitch + x;
#pragma unroll 4
        for (int t = 0; t < b.y; t++, p += pitch) {
            const uint32_t kv = (uint32_t)k[t];
#pragma unroll
            for (int c = 0; c < C; c++) {
                const uint32_t v = *(const uint32_t*)(p + (int64_t)c * plane);
#pragma unroll
                for (int j = 0; j < 4; j++) acc[c][j] += kv * ((v >> (8 * j)) & 255u);
            }
        }
    }
    uint32_t px[4][C];
#pragma unroll
    for (int j = 0; j < 4; j++) {
#pragma unroll
        for (int c = 0; c < C; c++) px[j][c] = im_clip8(acc[c][j]);
        if (C == 4 && o.unpremul) {
            const uint32_t a = px[j][C - 1];
            if (a != 0u && a != 255u)
#pragma unroll
                for (int c = 0; c < 3; c++) px[j][c] = min(255u * px[j][c] / a, 255u);
        }
    }
    const int nv = min(IM_VSTRIP, W - x0);                // pixels of this strip
    const int64_t at = (int64_t)y * W + x0;
    if (o.u8) {
        const uintptr_t g0 = (uintptr_t)(o.u8 + at * C), g1 = g0 + (uintptr_t)nv * C, a0 = g0 & ~(uintptr_t)3;
        const int head = (int)(g0 - a0), nd = (int)((g1 - a0 + 3) >> 2);
        uint8_t* obytes = (uint8_t*)ob + head;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (4 * lane + j < nv)
#pragma unroll
                for (int c = 0; c < C; c++) obytes[(4 * lane + j) * C + c] = (uint8_t)px[j][c];
        __syncthreads();
        for (int d = lane; d < nd; d += IM_VLANES) {
            const uintptr_t a = a0 + 4u * (uintptr_t)d;
            if (a >= g0 && a + 4 <= g1) *(uint32_t*)a = ob[d];
            else                                          // a dword shared with the strip next door, or with nothing: its bytes one by one
                for (int j = 0; j < 4; j++) if (a + j >= g0 && a + j < g1) *(uint8_t*)(a + j) = ((const uint8_t*)ob)[4 * d + j];
        }
    }
    if (o.planes || o.gray || o.mask) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            float q[C];
#pragma unroll
            for (int c = 0; c < C; c++) q[c] = fminf(fmaxf((float)px[j][c] / 255.0f, 0.0f), 1.0f);
            if (C >= 3) fb[3][4 * lane + j] = (0.2989f * q[0] + 0.587f * q[1]) + 0.114f * q[2];
            if (C == 4) fb[4][4 * lane + j] = q[C - 1];
#pragma unroll
            for (int c = 0; c < C; c++) fb[c < 3 ? c : 4][4 * lane + j] = (C == 4 && c < 3 && o.mask) ? q[c] * q[C - 1] : q[c];
        }
        __syncthreads();
        const int64_t HW = (int64_t)H * W;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = j * IM_VLANES + lane;
            if (i >= nv) continue;
            if (o.planes)
                for (int c = 0; c < o.n_planes; c++) o.planes[c * HW + at + i] = fb[c < 3 ? c : 4][i];
            if (o.gray) o.gray[at + i] = fb[3][i];
            if (o.mask) o.mask[at + i] = fb[4][i];
        }
    }
}

struct ImPlan {
    ImAxis ax, ay;
    int row0, rows, pitch;                                // the intermediate image: input rows [row0, row0 + rows), pitch bytes per row of a plane
    int2 *bounds_x, *bounds_y; int32_t *kk_x, *kk_y; uint8_t* mid;
    size_t bytes;
};
static bool im_sizes_ok(int32_t w, int32_t h, int32_t C, int32_t W, int32_t H)
{
    return w >= 1 && h >= 1 && W >= 1 && H >= 1 && (C == 1 || C == 3 || C == 4) && (int64_t)h * w * C < (1ll << 31) && (int64_t)H * W * C < (1ll << 31);
}
static ImPlan im_plan(int32_t w, int32_t h, int32_t C, int32_t W, int32_t H, void* base)
{
    ImPlan p;
    p.ax = im_axis(w, W); p.ay = im_axis(h, H);
    int n, last; double center;
    im_bounds(p.ay, 0, &p.row0, &n, &center);
    im_bounds(p.ay, H - 1, &last, &n, &center);
    p.rows = last + n - p.row0;
    p.pitch = (int)gsr_align((size_t)W, 128);
    GsrCarve c(base);
    p.bounds_x = c.take<int2>((size_t)W); p.kk_x = c.take<int32_t>((size_t)p.ax.K * W);
    p.bounds_y = c.take<int2>((size_t)H); p.kk_y = c.take<int32_t>((size_t)p.ay.K * H);
    p.mid = c.take<uint8_t>((size_t)C * p.rows * p.pitch);
    p.bytes = c.bytes();
    return p;
}

extern "C" size_t gsr_image_resample_scratch_bytes(int32_t w, int32_t h, int32_t C, int32_t W, int32_t H)
{
    return im_sizes_ok(w, h, C, W, H) ? im_plan(w, h, C, W, H, nullptr).bytes : 0;
}

template <int C>
static void im_launch(const ImPlan& p, const uint8_t* image, int64_t row_stride, int W, int H, int premul, uint32_t hstrips, uint32_t vstrips, ImOut o, hipStream_t s)
{
    const int64_t plane = (int64_t)p.rows * p.pitch;
    hipLaunchKernelGGL(k_img_hpass<C>, dim3((uint32_t)p.rows * hstrips), dim3(IM_HSTRIP), 0, s, image, row_stride, p.row0, W, hstrips, premul, (const int2*)p.bounds_x,
                       (const int32_t*)p.kk_x, p.mid, plane, p.pitch);
    hipLaunchKernelGGL(k_img_vpass<C>, dim3((uint32_t)H * vstrips), dim3(IM_VLANES), 0, s, (const uint8_t*)p.mid, plane, p.pitch, p.row0, W, H, vstrips,
                       (const int2*)p.bounds_y, (const int32_t*)p.kk_y, p.ay.K, o);
}

extern "C" int gsr_image_resample(const uint8_t* image, int32_t w, int32_t h, int32_t C, int64_t row_stride, int32_t W, int32_t H, uint8_t* out_u8, float* out_planes,
                                  int32_t n_planes, float* out_gray, float* out_mask, void* scratch, size_t scratch_bytes, void* stream)
{
    const char* who = "image_resample";
    if (!im_sizes_ok(w, h, C, W, H)) {
        gsr_set_error("%s: [%d, %d, %d] -> [%d, %d]: sizes from 1, 1, 3 or 4 channels, and fewer than 2^31 bytes on either side", who, h, w, C, H, W);
        return 1;
    }
    if (!image) { gsr_set_error("%s: null pointer", who); return 1; }
    if (row_stride < (int64_t)w * C) { gsr_set_error("%s: a row stride of %lld bytes for rows of %lld", who, (long long)row_stride, (long long)w * C); return 1; }
    if (C == 4 && (((uintptr_t)image | (uintptr_t)row_stride) & 3)) { gsr_set_error("%s: 4 channels: the image and its row stride must be multiples of 4 bytes", who); return 1; }
    if (out_planes && (n_planes < 1 || n_planes > C)) { gsr_set_error("%s: %d planes of an image of %d channels", who, n_planes, C); return 1; }
    if (out_gray && C < 3) { gsr_set_error("%s: the gray image needs 3 or 4 channels, the image has %d", who, C); return 1; }
    if (out_mask && (C != 4 || (out_planes && n_planes > 3))) { gsr_set_error("%s: the mask needs 4 channels and at most 3 planes", who); return 1; }
    const size_t need = gsr_image_resample_scratch_bytes(w, h, C, W, H);
    if (gsr_scratch_check(who, scratch, scratch_bytes, need)) return 1;
    const ImPlan p = im_plan(w, h, C, W, H, scratch);
    const uint32_t hstrips = gsr_div_up((uint32_t)W, IM_HSTRIP), vstrips = gsr_div_up((uint32_t)W, IM_VSTRIP);
    if ((int64_t)p.rows * hstrips >= (1ll << 31) || (int64_t)H * vstrips >= (1ll << 31)) { gsr_set_error("%s: more than 2^31 workgroups", who); return 1; }
    hipStream_t s = (hipStream_t)stream;
    const int premul = C == 4 && !(W == w && H == h);
    const uint32_t bx = gsr_div_up((uint32_t)W, IM_COEFF_BLOCK), by = gsr_div_up((uint32_t)H, IM_COEFF_BLOCK);
    hipLaunchKernelGGL(k_img_coeffs, dim3(bx + by), dim3(IM_COEFF_BLOCK), 0, s, p.ax, p.ay, bx, p.bounds_x, p.kk_x, p.bounds_y, p.kk_y);
    ImOut o;
    o.u8 = out_u8; o.planes = out_planes; o.gray = out_gray; o.mask = out_mask; o.n_planes = out_planes ? n_planes : 0; o.unpremul = premul;
    if (C == 1) im_launch<1>(p, image, row_stride, W, H, premul, hstrips, vstrips, o, s);
    else if (C == 3) im_launch<3>(p, image, row_stride, W, H, premul, hstrips, vstrips, o, s);
    else im_launch<4>(p, image, row_stride, W, H, premul, hstrips, vstrips, o, s);
    return gsr_check_launch(who, s, false);
}
