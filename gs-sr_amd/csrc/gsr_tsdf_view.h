// gsr_tsdf_view.h -- the device view of a block-sparse TSDF volume (gsr_tsdf_sparse of include/gsrast.h) and its addressing helpers, shared by the
// integration / merge kernels (gsr_tsdf_sparse.hip) and the mesh extraction (gsr_tsdf_mesh.hip).
#pragma once
#include "gsr_common.h"

#define TS_RES 16
#define TS_VOX (TS_RES * TS_RES * TS_RES)
static constexpr unsigned long long TS_EMPTY = ~0ull;

#define TS_UNIT_FLOATS (5 * TS_VOX)      // a unit's record: tsdf plane, weight plane, three colour planes (80 KB)
struct SparseTsdf {
    unsigned long long* keys;      // [cap_hash] packed unit coordinate, TS_EMPTY when free
    int32_t* slot;                 // [cap_hash] pool index of the unit
    int32_t* coord;                // [cap_blocks][3]
    uint32_t* stamp;               // [cap_blocks] last frame that touched the unit
    int32_t* list;                 // [cap_blocks] units touched by the current frame
    int32_t* counters;             // [0] = units allocated, [1] = units in `list`, [2] = pool/hash overflow flag
    unsigned long long* mask;      // [cap_blocks][16] written-group bits (ABI 8)
    float* chunk[GSR_TSDF_MAX_CHUNKS];      // unit records in chunks of doubling size (ABI 8): growing a volume allocates a chunk, it never copies a voxel
    uint32_t chunk0_log2, cap_hash_log2, cap_blocks;
};
// unit b's record: chunk 0 holds units [0, 2^chunk0_log2), chunk c >= 1 the units [2^(chunk0_log2 + c - 1), 2^(chunk0_log2 + c))
__device__ __forceinline__ float* ts_unit(const SparseTsdf& v, int b)
{
    const uint32_t hi = (uint32_t)b >> v.chunk0_log2;
    const int c = hi ? 32 - __clz((int)hi) : 0;
    const uint32_t base = c ? (1u << (v.chunk0_log2 + c - 1)) : 0u;
    return v.chunk[c] + (size_t)((uint32_t)b - base) * TS_UNIT_FLOATS;
}

__host__ __device__ __forceinline__ unsigned long long ts_pack(int x, int y, int z)
{
    return ((unsigned long long)(uint32_t)(x + (1 << 20)) << 42) | ((unsigned long long)(uint32_t)(y + (1 << 20)) << 21) | (unsigned long long)(uint32_t)(z + (1 << 20));
}
__device__ __forceinline__ uint32_t ts_hash(unsigned long long k, uint32_t log2cap) { return (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> (64 - log2cap)); }

__device__ __forceinline__ int ts_find(const SparseTsdf& v, int x, int y, int z)
{
    const unsigned long long key = ts_pack(x, y, z);
    const uint32_t mask = (1u << v.cap_hash_log2) - 1u;
    uint32_t h = ts_hash(key, v.cap_hash_log2);
    for (uint32_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        const unsigned long long cur = v.keys[h];
        if (cur == key) return v.slot[h];
        if (cur == TS_EMPTY) return -1;
    }
    return -1;
}

// storage order of a unit plane (see gsr_tsdf_sparse.hip, "the voxel pass"): group = four consecutive z
__host__ __device__ __forceinline__ int ts_group(int x, int y, int z)
{
    return ((x >> 2) << 8) | ((y >> 2) << 6) | ((z >> 2) << 4) | (((x >> 1) & 1) << 3) | (((y >> 1) & 1) << 2) | ((x & 1) << 1) | (y & 1);
}
// the inverse for thread t of a 256-thread workgroup in round r (group t + 256 r): voxel (x, y, z0 .. z0 + 3)
struct TsLane { int lx, iy, iz0; };
__device__ __forceinline__ TsLane ts_lane(int t)
{
    TsLane l;
    l.lx = ((t >> 3) & 1) * 2 + ((t >> 1) & 1);
    l.iy = ((t >> 6) & 3) * 4 + ((t >> 2) & 1) * 2 + (t & 1);
    l.iz0 = ((t >> 4) & 3) * 4;
    return l;
}
__device__ __forceinline__ unsigned long long ts_uniform64(unsigned long long x)
{
    return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(x >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)x);
}
__device__ __forceinline__ void ts_unpack4(const float4 a, float* o) { o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; }

// ---- host side
static inline SparseTsdf make_view(const gsr_tsdf_sparse* s)
{
    SparseTsdf v;
    v.keys = (unsigned long long*)s->keys; v.slot = s->slot; v.coord = s->coord; v.stamp = s->stamp; v.list = s->list; v.counters = s->counters;
    v.mask = (unsigned long long*)s->mask; v.cap_hash_log2 = s->cap_hash_log2; v.cap_blocks = s->cap_blocks; v.chunk0_log2 = s->chunk0_log2;
    for (int c = 0; c < GSR_TSDF_MAX_CHUNKS; c++) v.chunk[c] = c < (int)s->n_chunks ? s->chunk[c] : nullptr;
    return v;
}
static inline int check_vol(const gsr_tsdf_sparse* s)
{
    if (!s || !s->keys || !s->slot || !s->coord || !s->stamp || !s->list || !s->counters || !s->mask) {
        gsr_set_error("tsdf_sparse: null volume buffers"); return 1;
    }
    // (the shift count is checked first: chunk0_log2 + n_chunks - 1 can reach 50, and a 32-bit shift by 32 or more is undefined -- on x86 it wraps)
    if (s->n_chunks < 1 || s->n_chunks > GSR_TSDF_MAX_CHUNKS || s->chunk0_log2 > 27 || s->chunk0_log2 + s->n_chunks - 1 > 31 ||
        s->cap_blocks != (1u << (s->chunk0_log2 + s->n_chunks - 1))) {
        gsr_set_error("tsdf_sparse: %u chunks of first size 2^%u do not make a pool of %u units (chunk c >= 1 holds 2^(chunk0_log2 + c - 1) units)", s->n_chunks, s->chunk0_log2,
                      s->cap_blocks); return 1;
    }
    for (uint32_t c = 0; c < s->n_chunks; c++)
        if (!s->chunk[c]) { gsr_set_error("tsdf_sparse: null chunk %u", c); return 1; }
    if (s->cap_hash_log2 < 4 || s->cap_hash_log2 > 30 || s->cap_blocks == 0 || (1ull << s->cap_hash_log2) < 2ull * s->cap_blocks) {
        gsr_set_error("tsdf_sparse: hash table must hold at least twice the unit capacity"); return 1;
    }
    if (!(s->voxel_length > 0.f) || !(s->sdf_trunc > 0.f)) { gsr_set_error("tsdf_sparse: voxel_length / sdf_trunc must be positive"); return 1; }
    // a depth sample opens the units its +-sdf_trunc box overlaps, at most 4 per axis: a wider band would be dropped sample by sample
    if (2.0f * s->sdf_trunc > 3.0f * TS_RES * s->voxel_length) {
        gsr_set_error("tsdf_sparse: sdf_trunc %g exceeds 1.5 units (%g = 24 voxels): the truncation band must fit in 4 units per axis", s->sdf_trunc,
                      1.5f * TS_RES * s->voxel_length); return 1;
    }
    return 0;
}
