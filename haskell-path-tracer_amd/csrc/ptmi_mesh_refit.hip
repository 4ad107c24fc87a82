// ptmi_mesh_refit.hip -- moving a mesh scene's vertices on the device (ptmi_update_mesh_vertices): the triangle hierarchy keeps its
// topology (child references, leaf order) and gets new boxes; both copies of the triangle records are rewritten.  Three kernels:
//   mesh_refit_check_kernel    reads the new vertices only: refuses what mesh_build refuses (and a triangle in no leaf that would gain
//                              area) and reduces the box of the leaf triangles' vertices -- nothing of the scene is written;
//   mesh_refit_records_kernel  (v0, nx) (v1, ny) (v2, nz) by original index and in leaf order, by mesh_build's operations;
//   mesh_refit_level_kernel    the boxes of one level of the hierarchy, launched once per level, the deepest first: a node's children
//                              are complete when its launch starts (stream order), so no workgroup ever waits for another.
// The box arithmetic is ptmi_mesh_box.h's, which mesh_build and ptmi_mesh_refit_layout run on the host: the nodes are theirs bit for bit.
#include "ptmi_device.h"
#include "ptmi_mesh_box.h"

namespace ptmi {

namespace {

constexpr int kVertexFloats = 9;                          // per triangle: v0 v1 v2
constexpr int kChunkFloats = kVertexFloats * kBlock;     // a workgroup's triangles: 576 float4
constexpr unsigned int kCheckBlocks = 512;                // the check's grid: two workgroups per compute unit walk the chunks

// The 9 floats of kBlock consecutive triangles, fetched 16 bytes per lane into LDS (a triangle's 36 bytes are not 16-byte aligned; a
// chunk's 9216 are); every lane then reads its own triangle at a stride of 9 words: no bank conflict.  Nothing beyond total_floats is read.
__device__ __forceinline__ void stage_vertices(const float *v, long long first_float, long long total_floats, int aligned16, float *lds)
{
    for (int j = threadIdx.x; j < kChunkFloats / 4; j += kBlock) {
        const long long f = first_float + 4ll * j;
        if (aligned16 && f + 3 < total_floats) {
            *reinterpret_cast<float4 *>(lds + 4 * j) = *reinterpret_cast<const float4 *>(v + f);
        } else {
            for (int k = 0; k < 4; ++k)
                if (f + k < total_floats) lds[4 * j + k] = v[f + k];
        }
    }
    __syncthreads();
}

__global__ void __launch_bounds__(kBlock) mesh_refit_check_kernel(const float *vertices, int n, const int32_t *leaf_pos, unsigned int *result, int aligned16)
{
    __shared__ float lds[kChunkFloats];
    const long long total = (long long)n * kVertexFloats;
    const long long chunks = ((long long)n + kBlock - 1) / kBlock;
    unsigned int err = 0xffffffffu;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = __builtin_inff(); hi[a] = -__builtin_inff(); }
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        stage_vertices(vertices, ch * kChunkFloats, total, aligned16, lds);
        const long long i = ch * kBlock + threadIdx.x;
        if (i < n) {
            float v[3][3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int a = 0; a < 3; ++a) v[k][a] = lds[kVertexFloats * threadIdx.x + 3 * k + a];
            const TriangleNormal tn = triangle_normal(v[0], v[1], v[2]);
            const int pos = leaf_pos[i];
            const unsigned int key = (unsigned int)i << 2;
            unsigned int mine = 0xffffffffu;
            if (!tn.vertices_finite) mine = key | kRefitBadVertex;
            else if (!tn.finite) mine = key | kRefitBadNormal;
            else if (pos < 0 && tn.nn > 0.0f) mine = key | kRefitGainsArea;
            err = mine < err ? mine : err;
            if (pos >= 0) {
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int a = 0; a < 3; ++a) { lo[a] = __builtin_fminf(lo[a], v[k][a]); hi[a] = __builtin_fmaxf(hi[a], v[k][a]); }
            }
        }
        __syncthreads();                                   // the next chunk overwrites the staged one
    }
    // the wave's six extrema and its error word: one atomic each per wave, on order-preserving integer images of the floats
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)err, off);
        err = other < err ? other : err;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = __builtin_fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = __builtin_fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (err != 0xffffffffu) atomicMin(&result[kRefitError], err);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] <= hi[a]) {                          // (a wave without a leaf triangle, or with a NaN, adds nothing)
                atomicMin(&result[kRefitLo + a], ordered_image(lo[a]));
                atomicMax(&result[kRefitHi + a], ordered_image(hi[a]));
            }
        }
    }
}

__global__ void __launch_bounds__(kBlock) mesh_refit_records_kernel(const float *vertices, int n, const int32_t *leaf_pos, float4 *by_index, float4 *geom,
                                                                    int aligned16)
{
    __shared__ float lds[kChunkFloats];
    stage_vertices(vertices, (long long)blockIdx.x * kChunkFloats, (long long)n * kVertexFloats, aligned16, lds);
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < n;
    float v[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) v[k][a] = in ? lds[kVertexFloats * threadIdx.x + 3 * k + a] : 0.0f;
    const TriangleNormal tn = triangle_normal(v[0], v[1], v[2]);
    // the unit normal as mesh_build derives it: IEEE sqrt, three IEEE divisions; zero area: a NaN normal, never hit
    const float len = sqrt_rn(tn.nn);                      // (every lane of the wave is here: sqrt_rn votes)
    float nx = u2f(0x7fc00000u), ny = nx, nz = nx;
    if (tn.nn > 0.0f) { nx = tn.n[0] / len; ny = tn.n[1] / len; nz = tn.n[2] / len; }
    if (!in) return;
    const float4 r0 = float4{v[0][0], v[0][1], v[0][2], nx}, r1 = float4{v[1][0], v[1][1], v[1][2], ny}, r2 = float4{v[2][0], v[2][1], v[2][2], nz};
    float4 *q = by_index + 3 * (size_t)i;
    q[0] = r0; q[1] = r1; q[2] = r2;
    const int pos = leaf_pos[i];
    if (pos >= 0) {
        float4 *g = geom + 3 * (size_t)pos;
        g[0] = r0; g[1] = r1; g[2] = r2;
    }
}

// One lane per node of the level: both children's boxes from what lies under them -- a leaf's triangles (the records in leaf order,
// rewritten before), or the two stored boxes of the inner node below (an earlier launch's) -- and three 16-byte stores.
__global__ void __launch_bounds__(kBlock) mesh_refit_level_kernel(float4 *nodes, const float4 *geom, const int32_t *level_nodes, int count)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    float4 *nd = nodes + 4 * (size_t)level_nodes[k];
    const float4 links = nd[3];
    const int32_t ref[2] = {(int32_t)f2u(links.x), (int32_t)f2u(links.y)};
    float center[2][3], half[2][3];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (ref[c] == -1) {                                // an empty child keeps mesh_build's (0, -1)
            for (int a = 0; a < 3; ++a) { center[c][a] = 0.0f; half[c][a] = -1.0f; }
            continue;
        }
        double l[3], h[3];
        box_empty(l, h);
        if (ref[c] >= 0) {
            const float4 *in = nodes + 4 * (size_t)ref[c];
            const float4 a0 = in[0], a1 = in[1], a2 = in[2], a3 = in[3];
            const float c0[3] = {a0.x, a0.y, a0.z}, c1[3] = {a0.w, a1.x, a1.y}, h0[3] = {a1.z, a1.w, a2.x}, h1[3] = {a2.y, a2.z, a2.w};
            if ((int32_t)f2u(a3.x) != -1) box_join_stored(l, h, c0, h0);
            if ((int32_t)f2u(a3.y) != -1) box_join_stored(l, h, c1, h1);
        } else {
            const uint32_t leaf = (uint32_t)(-1 - ref[c]);
            const uint32_t first = leaf >> 8, end = first + (leaf & 255u);
            for (uint32_t t = first; t < end; ++t) {
                const float4 g0 = geom[3 * (size_t)t], g1 = geom[3 * (size_t)t + 1], g2 = geom[3 * (size_t)t + 2];
                const float v0[3] = {g0.x, g0.y, g0.z}, v1[3] = {g1.x, g1.y, g1.z}, v2[3] = {g2.x, g2.y, g2.z};
                double tl[3], th[3];
                triangle_box(v0, v1, v2, tl, th);
                box_join(l, h, tl, th);
            }
        }
        box_store(center[c], half[c], l, h);
    }
    nd[0] = float4{center[0][0], center[0][1], center[0][2], center[1][0]};
    nd[1] = float4{center[1][1], center[1][2], half[0][0], half[0][1]};
    nd[2] = float4{half[0][2], half[1][0], half[1][1], half[1][2]};
}

}  // namespace

hipError_t launch_mesh_refit_check(const float *vertices, int n, const int32_t *leaf_pos, unsigned int *result, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned int chunks = blocks_for(n);
    return launch(mesh_refit_check_kernel, dim3(chunks < kCheckBlocks ? chunks : kCheckBlocks), dim3(kBlock), 0, stream, vertices, n, leaf_pos, result,
                  ((uintptr_t)vertices & 15u) == 0 ? 1 : 0);
}

hipError_t launch_mesh_refit_records(const float *vertices, int n, const int32_t *leaf_pos, float4 *by_index, float4 *geom, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return launch(mesh_refit_records_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, vertices, n, leaf_pos, by_index, geom,
                  ((uintptr_t)vertices & 15u) == 0 ? 1 : 0);
}

hipError_t launch_mesh_refit_level(float4 *nodes, const float4 *geom, const int32_t *level_nodes, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    return launch(mesh_refit_level_kernel, dim3(blocks_for(count)), dim3(kBlock), 0, stream, nodes, geom, level_nodes, count);
}

}  // namespace ptmi
