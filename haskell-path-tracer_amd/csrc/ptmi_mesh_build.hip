// ptmi_mesh_build.hip -- giving a mesh scene NEW triangles on the device (ptmi_set_mesh_triangles): validation, the leaf order and
// every derived block, from ptmi_triangle records in device memory.  The kernels, in the order of their launches:
//   mesh_build_check_kernel            reads the triangles only: refuses what mesh_build and ptmi_set_scene_mesh refuse, counts the kept
//                                      (non-zero-area) triangles, reduces the box of their vertices, finds GLASS -- writes `result` alone;
//   mesh_build_keys_kernel             (after the host has read the box) the Morton key of every triangle (ptmi_mesh_morton.h), bit 42
//                                      for a triangle in no leaf, and its index;
//   mesh_build_sort_histogram_kernel   a least-significant-digit radix sort of (key, index), 8 bits per pass: per tile of 4096 items the
//   mesh_build_sort_scan_kernel        digit counts; their exclusive scan in (digit, tile) order, one workgroup; the stable scatter, ranks
//   mesh_build_sort_scatter_kernel     within a wave by ballot / mbcnt and across a tile's waves and rounds in order -- no atomics;
//   mesh_build_order_kernel            leaf_pos of every triangle and the order block from the sorted indices;
//   mesh_build_scatter_kernel          the records by index and in leaf order (mesh_build's operations, as the refit's records kernel)
//                                      and the material tail of the scene block.
// Every dependency is a launch boundary in stream order: no workgroup waits for another.  The boxes are ptmi_mesh_refit.hip's level
// kernel over the topology of the kept count.
#include "ptmi_device.h"
#include "ptmi_mesh_box.h"
#include "ptmi_mesh_morton.h"

namespace ptmi {

namespace {

constexpr int kTriFloats = 15;                            // a ptmi_triangle
constexpr int kChunkFloats = kTriFloats * kBlock;        // a workgroup's triangles: 960 float4
constexpr unsigned int kCheckBlocks = 512;                // the check's grid: two workgroups per compute unit walk the chunks
constexpr int kSortRounds = 16;                           // a sort tile: kSortRounds rounds of kBlock items
constexpr int kSortTile = kSortRounds * kBlock;
constexpr int kDigits = 256;
constexpr int kWaves = kBlock / 64;

// The 15 floats of kBlock consecutive triangles, fetched 16 bytes per lane into LDS (a triangle's 60 bytes are not 16-byte aligned; a
// chunk's 15360 are); every lane then reads its own triangle at a stride of 15 words: no bank conflict.  Nothing beyond total_floats is read.
__device__ __forceinline__ void stage_triangles(const float *v, long long first_float, long long total_floats, int aligned16, float *lds)
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

__device__ __forceinline__ void staged_vertices(const float *lds, float v[3][3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) v[k][a] = lds[kTriFloats * threadIdx.x + 3 * k + a];
}

__global__ void __launch_bounds__(kBlock) mesh_build_check_kernel(const float *triangles, int n, unsigned int *result, int aligned16)
{
    __shared__ float lds[kChunkFloats];
    const long long total = (long long)n * kTriFloats;
    const long long chunks = ((long long)n + kBlock - 1) / kBlock;
    unsigned int err = 0xffffffffu, kept = 0, glass = 0;
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) { lo[a] = __builtin_inff(); hi[a] = -__builtin_inff(); }
    for (long long ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        stage_triangles(triangles, ch * kChunkFloats, total, aligned16, lds);
        const long long i = ch * kBlock + threadIdx.x;
        if (i < n) {
            float v[3][3];
            staged_vertices(lds, v);
            const float *m = lds + kTriFloats * threadIdx.x + 9;      // colour[3], illuminance, brdf_tag, brdf_param
            const bool material_finite = finite_f32(m[0]) && finite_f32(m[1]) && finite_f32(m[2]) && finite_f32(m[3]) && finite_f32(m[5]);
            const int32_t tag = (int32_t)f2u(m[4]);
            const TriangleNormal tn = triangle_normal(v[0], v[1], v[2]);
            const unsigned int key = (unsigned int)i << 2;
            unsigned int mine = 0xffffffffu;
            if (!tn.vertices_finite) mine = key | kBuildBadVertex;
            else if (!material_finite) mine = key | kBuildBadMaterial;
            else if (!tn.finite) mine = key | kBuildBadNormal;
            else if (tag < PTMI_MATTE || tag > PTMI_GLASS) mine = key | kBuildBadTag;
            err = mine < err ? mine : err;
            glass |= tag == PTMI_GLASS ? 1u : 0u;
            if (tn.nn > 0.0f) {
                ++kept;
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int a = 0; a < 3; ++a) { lo[a] = __builtin_fminf(lo[a], v[k][a]); hi[a] = __builtin_fmaxf(hi[a], v[k][a]); }
            }
        }
        __syncthreads();                                   // the next chunk overwrites the staged one
    }
    // the wave's six extrema, its error word and its counts: one atomic each per wave
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int other = (unsigned int)__shfl_xor((int)err, off);
        err = other < err ? other : err;
        kept += (unsigned int)__shfl_xor((int)kept, off);
        glass |= (unsigned int)__shfl_xor((int)glass, off);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lo[a] = __builtin_fminf(lo[a], __shfl_xor(lo[a], off));
            hi[a] = __builtin_fmaxf(hi[a], __shfl_xor(hi[a], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (err != 0xffffffffu) atomicMin(&result[kBuildError], err);
        if (kept) atomicAdd(&result[kBuildKept], kept);
        if (glass) atomicOr(&result[kBuildGlass], 1u);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo[a] <= hi[a]) {                          // (a wave without a kept triangle, or with a NaN, adds nothing)
                atomicMin(&result[kBuildLo + a], ordered_image(lo[a]));
                atomicMax(&result[kBuildHi + a], ordered_image(hi[a]));
            }
        }
    }
}

struct MortonBox { float lo[3], hi[3]; };

__global__ void __launch_bounds__(kBlock) mesh_build_keys_kernel(const float *triangles, int n, MortonBox box, uint64_t *keys, uint32_t *indices, int aligned16)
{
    __shared__ float lds[kChunkFloats];
    stage_triangles(triangles, (long long)blockIdx.x * kChunkFloats, (long long)n * kTriFloats, aligned16, lds);
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float v[3][3];
    staged_vertices(lds, v);
    const TriangleNormal tn = triangle_normal(v[0], v[1], v[2]);
    keys[i] = tn.nn > 0.0f ? morton_key(v[0], v[1], v[2], box.lo, box.hi) : kMortonNoLeaf;
    indices[i] = (uint32_t)i;
}

// counts[tile * 256 + digit]: how many of the tile's keys hold the digit
__global__ void __launch_bounds__(kBlock) mesh_build_sort_histogram_kernel(const uint64_t *keys, int n, int shift, unsigned int *counts)
{
    __shared__ unsigned int hist[kDigits];
    hist[threadIdx.x] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {
        const long long g = first + (long long)r * kBlock + threadIdx.x;
        if (g < n) atomicAdd(&hist[(unsigned int)(keys[g] >> shift) & (kDigits - 1)], 1u);       // (LDS: a count, whatever the order)
    }
    __syncthreads();
    counts[(size_t)blockIdx.x * kDigits + threadIdx.x] = hist[threadIdx.x];
}

// In place: counts[tile][digit] -> where the tile's first key with the digit goes: every smaller digit of every tile, then the digit
// of the tiles before.  ONE workgroup; lane d walks digit d's column (coalesced across the lanes).
__global__ void __launch_bounds__(kBlock) mesh_build_sort_scan_kernel(unsigned int *counts, int tiles)
{
    __shared__ unsigned int total[kDigits];
    const int d = threadIdx.x;
    unsigned int sum = 0;
    for (int t = 0; t < tiles; ++t) {
        const unsigned int c = counts[(size_t)t * kDigits + d];
        counts[(size_t)t * kDigits + d] = sum;
        sum += c;
    }
    total[d] = sum;
    __syncthreads();
    for (int step = 1; step < kDigits; step <<= 1) {       // inclusive scan of the 256 totals
        const unsigned int below = d >= step ? total[d - step] : 0u;
        __syncthreads();
        total[d] += below;
        __syncthreads();
    }
    const unsigned int base = total[d] - sum;
    for (int t = 0; t < tiles; ++t) counts[(size_t)t * kDigits + d] += base;
}

// The stable scatter of one tile: its keys in their order, round by round, wave by wave, lane by lane.  A lane's rank among the lanes
// of its wave with the same digit is a count of lower lanes in the match mask (eight ballots); the waves' counts of the round meet in
// LDS; `running` carries the digit's position from round to round.  Nothing is written at or beyond n.
__global__ void __launch_bounds__(kBlock) mesh_build_sort_scatter_kernel(const uint64_t *keys, const uint32_t *indices, int n, int shift,
                                                                         const unsigned int *offsets, uint64_t *keys_out, uint32_t *indices_out)
{
    __shared__ unsigned int running[kDigits];
    __shared__ unsigned int count[kWaves][kDigits];
    const int wave = threadIdx.x >> 6;
    running[threadIdx.x] = offsets[(size_t)blockIdx.x * kDigits + threadIdx.x];
#pragma unroll
    for (int w = 0; w < kWaves; ++w) count[w][threadIdx.x] = 0;
    __syncthreads();
    const long long first = (long long)blockIdx.x * kSortTile;
    for (int r = 0; r < kSortRounds; ++r) {
        const long long g = first + (long long)r * kBlock + threadIdx.x;
        const bool valid = g < n;
        const uint64_t key = valid ? keys[g] : 0;
        const uint32_t index = valid ? indices[g] : 0;
        const unsigned int digit = (unsigned int)(key >> shift) & (kDigits - 1);
        uint64_t same = __builtin_amdgcn_ballot_w64(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (digit >> b) & 1u;
            const uint64_t with = __builtin_amdgcn_ballot_w64(bit);
            same &= bit ? with : ~with;
        }
        const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)same, 0u));
        if (valid && rank == 0) count[wave][digit] = (unsigned int)__builtin_popcountll(same);
        __syncthreads();
        if (valid) {
            unsigned int at = running[digit] + rank;
            for (int w = 0; w < wave; ++w) at += count[w][digit];
            if (at < (unsigned int)n) { keys_out[at] = key; indices_out[at] = index; }
        }
        __syncthreads();
        unsigned int all = 0;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) { all += count[w][threadIdx.x]; count[w][threadIdx.x] = 0; }
        running[threadIdx.x] += all;
        __syncthreads();
    }
}

// sorted: the triangles' indices by (key, index), the n_kept leaf triangles first
__global__ void __launch_bounds__(kBlock) mesh_build_order_kernel(const uint32_t *sorted, int n, int n_kept, int32_t *leaf_pos, int32_t *order)
{
    const long long pos = (long long)blockIdx.x * kBlock + threadIdx.x;
    if (pos >= n) return;
    const uint32_t i = sorted[pos];
    if (i >= (uint32_t)n) return;
    leaf_pos[i] = pos < n_kept ? (int32_t)pos : -1;
    if (pos < n_kept) order[pos] = (int32_t)i;
}

__global__ void __launch_bounds__(kBlock) mesh_build_scatter_kernel(const float *triangles, int n, int n_kept, const int32_t *leaf_pos, float4 *by_index,
                                                                    float4 *geom, float4 *materials, int aligned16)
{
    __shared__ float lds[kChunkFloats];
    stage_triangles(triangles, (long long)blockIdx.x * kChunkFloats, (long long)n * kTriFloats, aligned16, lds);
    const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
    const bool in = i < n;
    float v[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int a = 0; a < 3; ++a) v[k][a] = in ? lds[kTriFloats * threadIdx.x + 3 * k + a] : 0.0f;
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
    if (pos >= 0 && pos < n_kept) {
        float4 *g = geom + 3 * (size_t)pos;
        g[0] = r0; g[1] = r1; g[2] = r2;
    }
    // (colour, illuminance) (tag, p, p / pi, 0.5 (1 - p)): ptmi_set_scene_mesh's pair, each operation rounded on its own
    const float *m = lds + kTriFloats * threadIdx.x + 9;
    const float p = m[5];
    materials[2 * (size_t)i] = float4{m[0], m[1], m[2], m[3]};
    materials[2 * (size_t)i + 1] = float4{m[4], p, p / kPi, 0.5f * (1.0f - p)};
}

int aligned(const void *p) { return ((uintptr_t)p & 15u) == 0 ? 1 : 0; }

}  // namespace

hipError_t launch_mesh_build_check(const float *triangles, int n, unsigned int *result, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    const unsigned int chunks = blocks_for(n);
    return launch(mesh_build_check_kernel, dim3(chunks < kCheckBlocks ? chunks : kCheckBlocks), dim3(kBlock), 0, stream, triangles, n,
                  result, aligned(triangles));
}

size_t mesh_build_sort_bytes(int n)
{
    const size_t m = (size_t)(n > 0 ? n : 1), tiles = (m + kSortTile - 1) / kSortTile;
    return 2 * m * sizeof(uint64_t) + 2 * m * sizeof(uint32_t) + tiles * kDigits * sizeof(unsigned int);
}

// The radix sort of n (key, index) pairs that lie in `scratch` (sort_keys / sort_indices of ptmi_kernels.h; mesh_build_sort_bytes(n)
// bytes), ascending by key, equal keys in their order: six passes over bits 0 .. 47.  *sorted: where the sorted indices are afterwards.
hipError_t launch_sort_pairs(void *scratch, int n, const uint32_t **sorted, hipStream_t stream)
{
    const size_t m = (size_t)n;
    const int tiles = (int)((m + kSortTile - 1) / kSortTile);
    uint64_t *keys[2] = {sort_keys(scratch, n), sort_keys(scratch, n) + m};
    uint32_t *indices[2] = {sort_indices(scratch, n), sort_indices(scratch, n) + m};
    unsigned int *counts = indices[1] + m;
    hipError_t e = hipSuccess;
    int from = 0;
    for (int shift = 0; shift <= kMortonKeyBits && e == hipSuccess; shift += 8, from ^= 1) {      // six passes: bits 0 .. 47
        e = launch(mesh_build_sort_histogram_kernel, dim3(tiles), dim3(kBlock), 0, stream, keys[from], n, shift, counts);
        if (e == hipSuccess) e = launch(mesh_build_sort_scan_kernel, dim3(1), dim3(kBlock), 0, stream, counts, tiles);
        if (e == hipSuccess)
            e = launch(mesh_build_sort_scatter_kernel, dim3(tiles), dim3(kBlock), 0, stream, keys[from], indices[from], n, shift, counts, keys[from ^ 1], indices[from ^ 1]);
    }
    *sorted = indices[from];
    return e;
}

hipError_t launch_mesh_build_order(const float *triangles, int n, int n_kept, const float lo[3], const float hi[3], void *scratch, int32_t *leaf_pos,
                                   int32_t *order, hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    MortonBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo[a]; box.hi[a] = hi[a]; }
    hipError_t e = launch(mesh_build_keys_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, triangles, n, box, sort_keys(scratch, n), sort_indices(scratch, n),
                          aligned(triangles));
    const uint32_t *sorted = nullptr;
    if (e == hipSuccess) e = launch_sort_pairs(scratch, n, &sorted, stream);
    if (e == hipSuccess) e = launch(mesh_build_order_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, sorted, n, n_kept, leaf_pos, order);
    return e;
}

hipError_t launch_mesh_build_scatter(const float *triangles, int n, int n_kept, const int32_t *leaf_pos, float4 *by_index, float4 *geom, float4 *materials,
                                     hipStream_t stream)
{
    if (n <= 0) return hipSuccess;
    return launch(mesh_build_scatter_kernel, dim3(blocks_for(n)), dim3(kBlock), 0, stream, triangles, n, n_kept, leaf_pos, by_index,
                  geom, materials, aligned(triangles));
}

}  // namespace ptmi
