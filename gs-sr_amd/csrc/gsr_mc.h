// gsr_mc.h -- the marching-cubes core shared by gsr_tsdf_mesh.hip (unit rows with neighbour bases) and gsr_unbounded.hip (packed words per
// lattice point): the case table in LDS, the case of a cube, its triangle count, the crossing parameter and the triangle loop.  What differs -- where
// a corner's value lies, how an edge names its vertex -- comes in as a callable.  Both units are built without FMA contraction: positions are compared bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#define GSR_MC_TABLE_QUAL static __constant__ const
#include "gsr_mc_table.h"

// the table's copy in LDS, a row = 16 bytes.  A workgroup of 256 threads stages it, one row each; the caller's next barrier publishes it.
__device__ __forceinline__ void mc_stage_table(uint32_t (*tab)[4])
{
    reinterpret_cast<uint4*>(&tab[0][0])[threadIdx.x] = reinterpret_cast<const uint4*>(&GSR_MC_TABLE[0][0])[threadIdx.x];
}
// case bit i = corner i, at offset (i & 1, (i >> 1) & 1, (i >> 2) & 1), is inside: value < 0, a value of exactly 0 is outside
template <typename F> __device__ __forceinline__ int mc_case(F corner)
{
    int c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) c |= (corner(i) < 0.f ? 1 : 0) << i;
    return c;
}
__device__ __forceinline__ uint32_t mc_tris(const uint32_t (*tab)[4], int c) { return tab[c][3] >> 24; }
__device__ __forceinline__ uint32_t mc_tris_const(int c) { return GSR_MC_TABLE[c][15]; }      // without a staged table
// where the surface crosses the edge from a corner with value f0 to one with value f1, as a fraction of the edge
__device__ __forceinline__ float mc_cross(float f0, float f1) { return f0 / (f0 - f1); }
// The triangles of case c go to tris[3 ti ..] for ti = first, first + 1, ... while ti < limit; returns the ti behind the last.
// vertex_of(corner, axis) = the index of the vertex on the edge that leaves `corner` of the cube along `axis`.
template <typename I, typename F>
__device__ __forceinline__ I mc_triangles(const uint32_t (*tab)[4], int c, I ti, I limit, int32_t* __restrict__ tris, F vertex_of)
{
    const uint32_t ntri = mc_tris(tab, c);
    const uint8_t* e = reinterpret_cast<const uint8_t*>(&tab[c][0]);
    for (uint32_t j = 0; j < ntri; j++, ti++) {
        int32_t idx[3];
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int ed = e[3 * j + q];
            idx[q] = (int32_t)vertex_of((int)GSR_MC_EDGE_CORNER[ed], (int)GSR_MC_EDGE_AXIS[ed]);
        }
        if (ti < limit) { tris[3 * ti] = idx[0]; tris[3 * ti + 1] = idx[1]; tris[3 * ti + 2] = idx[2]; }
    }
    return ti;
}
