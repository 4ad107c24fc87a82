// ptmi_bvh_refit.hip -- moving (ptmi_update_spheres) and replacing (ptmi_set_bvh_spheres) the spheres of a BVH or mesh scene on the
// device.  The sphere hierarchy keeps or is given its topology on the host side (child references, leaf order: ptmi_api.cpp,
// ptmi_bvh_build.hip) and gets new boxes here.  The input is `words` floats per sphere by original index: 4 -- (x, y, z, radius) -- for
// an update, 10 -- a ptmi_sphere -- for a set.  Three kernels:
//   bvh_check_kernel    reads the new spheres only: refuses what bvh_build and the scene calls refuse, reduces the box of the centres and
//                       finds GLASS -- nothing of the scene is written;
//   bvh_records_kernel  one lane per position of the leaf order: (c, r * r) in leaf order and by original index (pack_scene's row), and
//                       for a set the material pair of the scene block, by pack_scene's operations;
//   bvh_level_kernel    the boxes and inv_2r of one level of the hierarchy, launched once per level, the deepest first: a node's children
//                       are complete when its launch starts (stream order), so no workgroup ever waits for another.
// The box arithmetic is ptmi_bvh_box.h's, which bvh_build and ptmi_bvh_refit_layout run on the host: the nodes are theirs bit for bit.
#include "ptmi_device.h"
#include "../../include/ptmi.h"
#include "ptmi_bvh_box.h"

namespace ptmi {

namespace {

constexpr unsigned int kCheckBlocks = 512;                // the check's grid: two workgroups per compute unit walk the chunks

// The kWords floats of kBlock consecutive spheres, fetched 16 bytes per lane into LDS (a ptmi_sphere's 40 bytes are not 16-byte aligned; a
// chunk's are); every lane then reads its own sphere.  Nothing beyond total_floats is read.
template <int kWords>
__device__ __forceinline__ void stage_spheres(const float *v, long long first_float, long long total_floats, int aligned16, float *lds)
{
    for (int j = threadIdx.x; j < kWords * kBlock / 4; j += kBlock) {
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

template <int kWords>
__global__ void __launch_bounds__(kBlock) bvh_check_kernel(const float *spheres, int n, unsigned int *result, int aligned16)
{
    __shared__ float lds[kWords * kBlock];
    const long long total = (long long)n * kWords;
    const long long chunks = ((long long)n + kBlock - 1) / kBlock;
    unsigned int err = 0xffffffffu, glass = 0;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = __builtin_inff(); hi[a] = -__builtin_inff(); }
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        stage_spheres<kWords>(spheres, ch * (kWords * kBlock), total, aligned16, lds);
        const long long i = ch * kBlock + threadIdx.x;
        if (i < n) {
            const float *s = lds + kWords * threadIdx.x;      // position[3], radius (, colour[3], illuminance, brdf_tag, brdf_param)
            const float r2 = s[3] * s[3];                     // what the device tests against (pack_scene)
            const unsigned int key = (unsigned int)i << 2;
            unsigned int mine = 0xffffffffu;
            if (!(finite_f32(s[0]) && finite_f32(s[1]) && finite_f32(s[2]) && finite_f32(s[3]) && finite_f32(r2))) mine = key | kSphBadGeometry;
            if (kWords == 10 && mine == 0xffffffffu) {
                const int32_t tag = (int32_t)f2u(s[8]);
                if (!(finite_f32(s[4]) && finite_f32(s[5]) && finite_f32(s[6]) && finite_f32(s[7]) && finite_f32(s[9]))) mine = key | kSphBadMaterial;
                else if (tag < PTMI_MATTE || tag > PTMI_GLASS) mine = key | kSphBadTag;
                glass |= tag == PTMI_GLASS ? 1u : 0u;
            }
            err = mine < err ? mine : err;
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = __builtin_fminf(lo[a], s[a]); hi[a] = __builtin_fmaxf(hi[a], s[a]); }
        }
        __syncthreads();                                   // the next chunk overwrites the staged one
    }
    // the wave's six extrema, its error word and its flag: one atomic each per wave, on order-preserving integer images of the floats
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)err, off);
        err = other < err ? other : err;
        glass |= (unsigned int)__shfl_xor((int)glass, off);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = __builtin_fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = __builtin_fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (err != 0xffffffffu) atomicMin(&result[kSphError], err);
        if (glass) atomicOr(&result[kSphGlass], 1u);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] <= hi[a]) {                          // (a wave without a sphere, or with a NaN, adds nothing)
                atomicMin(&result[kSphLo + a], ordered_image(lo[a]));
                atomicMax(&result[kSphHi + a], ordered_image(hi[a]));
            }
        }
    }
}

// (x, y, z, radius) of sphere i: one 16-byte load where the rows are 16 bytes wide and aligned, four 4-byte loads otherwise
template <int kWords>
__device__ __forceinline__ float4 sphere_geometry(const float *spheres, size_t i, int aligned16)
{
    if (kWords == 4 && aligned16) return reinterpret_cast<const float4 *>(spheres)[i];
    const float *s = spheres + kWords * i;
    return float4{s[0], s[1], s[2], s[3]};
}

// geom: the spheres in leaf order; scene: the packed scene block, sphere rows first; materials: its pair for sphere 0 (a set only)
template <int kWords>
__global__ void __launch_bounds__(kBlock) bvh_records_kernel(const float *spheres, int n, const int32_t *order, float4 *geom, float4 *scene,
                                                             float4 *materials, int aligned16)
{
    const long long k = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (k >= n) return;
    const uint32_t i = (uint32_t)order[k];
    if (i >= (uint32_t)n) return;                          // (never, for a leaf order: nothing is written out of bounds)
    const float4 g = sphere_geometry<kWords>(spheres, i, aligned16);
    const float4 row = float4{g.x, g.y, g.z, g.w * g.w};
    geom[k] = row;
    scene[i] = row;
    if (kWords == 10) {
        // (colour, illuminance) (tag, p, p / pi, 0.5 (1 - p)): pack_scene's pair, each operation rounded on its own
        const float *m = spheres + (size_t)kWords * i + 4;
        const float p = m[5];
        materials[2 * (size_t)i] = float4{m[0], m[1], m[2], m[3]};
        materials[2 * (size_t)i + 1] = float4{m[4], p, p / kPi, 0.5f * (1.0f - p)};
    }
}

// One lane per node of the level: both children's boxes and inv_2r from what lies under them -- a leaf's spheres (the new geometry
// through the leaf order), or the two stored boxes of the inner node below (an earlier launch's) -- and four 16-byte stores.
template <int kWords>
__global__ void __launch_bounds__(kBlock) bvh_level_kernel(float4 *nodes, const float *spheres, int n, const int32_t *order, const int32_t *level_nodes,
                                                           int count, int aligned16)
{
    const int k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= count) return;
    float4 *nd = nodes + 4 * (size_t)level_nodes[k];
    const float4 links = nd[3];
    const int32_t ref[2] = {(int32_t)f2u(links.x), (int32_t)f2u(links.y)};
    float center[2][3], half[2][3], inv_2r[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (ref[c] == -1) {
            bvh_empty_child(center[c], half[c], inv_2r[c]);
            continue;
        }
        double l[3], h[3];
        if (ref[c] >= 0) {
            const float4 *in = nodes + 4 * (size_t)ref[c];
            const float4 a0 = in[0], a1 = in[1], a2 = in[2], a3 = in[3];
            const float ic[2][3] = {{a0.x, a0.y, a0.z}, {a0.w, a1.x, a1.y}}, ih[2][3] = {{a1.z, a1.w, a2.x}, {a2.y, a2.z, a2.w}};
            const int32_t r0 = (int32_t)f2u(a3.x), r1 = (int32_t)f2u(a3.y);
            bvh_inner_box(l, h, ic, ih, r0, r1);
            inv_2r[c] = bvh_inner_inv_2r(a3.z, a3.w, r0, r1);
        } else {
            const uint32_t leaf = (uint32_t)(-1 - ref[c]);
            const uint32_t first = leaf >> 8, end = first + (leaf & 255u);
            double r_min = __builtin_inf();
            box_empty(l, h);
            for (uint32_t t = first; t < end && t < (uint32_t)n; ++t) {
                const uint32_t i = (uint32_t)order[t];
                if (i >= (uint32_t)n) continue;
                const float4 g = sphere_geometry<kWords>(spheres, i, aligned16);
                const float p[3] = {g.x, g.y, g.z};
                bvh_leaf_join(l, h, r_min, p, g.w);
            }
            inv_2r[c] = bvh_leaf_inv_2r(r_min);
        }
        bvh_store(center[c], half[c], l, h);
    }
    nd[0] = float4{center[0][0], center[0][1], center[0][2], center[1][0]};
    nd[1] = float4{center[1][1], center[1][2], half[0][0], half[0][1]};
    nd[2] = float4{half[0][2], half[1][0], half[1][1], half[1][2]};
    nd[3] = float4{links.x, links.y, inv_2r[0], inv_2r[1]};
}

int aligned(const void *p) { return ((uintptr_t)p & 15u) == 0 ? 1 : 0; }

}  // namespace

hipError_t launch_bvh_check(const float *spheres, int words, int n, unsigned int *result, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned int chunks = blocks_for(n);
    const dim3 grid(chunks < kCheckBlocks ? chunks : kCheckBlocks);
    if (words == 4) return launch(bvh_check_kernel<4>, grid, dim3(kBlock), 0, stream, spheres, n, result, aligned(spheres));
    return launch(bvh_check_kernel<10>, grid, dim3(kBlock), 0, stream, spheres, n, result, aligned(spheres));
}

hipError_t launch_bvh_records(const float *spheres, int words, int n, const int32_t *order, float4 *geom, float4 *scene, float4 *materials, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    if (words == 4) return launch(bvh_records_kernel<4>, dim3(blocks_for(n)), dim3(kBlock), 0, stream, spheres, n, order, geom, scene, materials, aligned(spheres));
    return launch(bvh_records_kernel<10>, dim3(blocks_for(n)), dim3(kBlock), 0, stream, spheres, n, order, geom, scene, materials, aligned(spheres));
}

hipError_t launch_bvh_level(float4 *nodes, const float *spheres, int words, int n, const int32_t *order, const int32_t *level_nodes, int count, hipStream_t stream)
{
    if (count <= 0) return hipSuccess;
    if (words == 4)
        return launch(bvh_level_kernel<4>, dim3(blocks_for(count)), dim3(kBlock), 0, stream, nodes, spheres, n, order, level_nodes, count, aligned(spheres));
    return launch(bvh_level_kernel<10>, dim3(blocks_for(count)), dim3(kBlock), 0, stream, nodes, spheres, n, order, level_nodes, count, aligned(spheres));
}

}  // namespace ptmi
