// The chunk-table walk of the one-launch-over-many-tensors kernels: calm_cast_bf16 (spectral.hip), calm_optim_step
// (optim.hip), calm_ema_update / calm_ema_swap (ema.hip), calm_snapshot_pack / _unpack (snapshot.hip).  The host
// (backend.chunk_table) writes one record per tensor into a device table and cuts every tensor into chunks of CHUNK_ELEMS
// elements: chunk_entry[k] = record of chunk k, record.chunk0 = its first chunk.  One workgroup per chunk, every element
// in one thread of one workgroup: a kernel's result per element does not depend on the grid.
#pragma once
#include "common.h"

constexpr int CHUNK_ELEMS = 16384;           // elements (4-byte words) per work item: 64 per thread of a 256-thread workgroup
static_assert(CHUNK_ELEMS % 4 == 0, "the vector paths start every chunk on a multiple of 4 elements");

// A pointer read out of the table is a generic one to the compiler (flat_load / flat_store); these say it is device memory
// (global_load / global_store: one wait counter, no aperture check).
#define CALM_GLOBAL __attribute__((address_space(1)))
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef CALM_GLOBAL float gf32;
typedef CALM_GLOBAL f32x4 gf32x4;
typedef CALM_GLOBAL uint32_t gu32;
typedef CALM_GLOBAL u32x4 gu32x4;

__device__ __forceinline__ bool dev_aligned16(const CALM_GLOBAL void* p) { return ((uintptr_t)p & 15u) == 0; }

// [i0, i1) of chunk `chunk` (the kernel's blockIdx.x) of an entry of `len` elements whose first chunk is `chunk0`.  An
// unsigned chunk in front of chunk0 (a table the host never builds) wraps to an empty span; snapshot_move passes an int
// and refuses i0 < 0 itself.
struct ChunkSpan { long i0, i1; };
template <class Index>
__device__ __forceinline__ ChunkSpan chunk_span(Index chunk, int chunk_len, int chunk0, long len) {
    const long i0 = (long)(chunk - chunk0) * chunk_len;
    return {i0, min(i0 + (long)chunk_len, len)};
}
// chunks of an entry of `len` elements: what the host counted from chunk0 on
__device__ __forceinline__ int chunk_count(int chunk_len, long len) { return (int)((len + chunk_len - 1) / chunk_len); }

// The deferred spectral-norm coefficient c = <G, W_orig> / sigma of a tensor of calm_optim_step's table, in the two steps
// calm_grad_accum, calm_grad_stats and calm_sam_perturb share, so that c has in all of them the bits calm_optim_step gives
// it (optim_stats forms the same partial next to its other sums).  256-thread workgroups.
// Step 1, one workgroup per chunk [i0, i1): thread t adds the elements i0 + t, i0 + t + 256, ... serially, then
// block_sum_256 (red: four floats of LDS); every thread returns the chunk's partial.
__device__ __forceinline__ float chunk_gw_partial(const calm_optim_tensor& e, long i0, long i1, float* red) {
    float gw = 0.f;
    for (long i = i0 + threadIdx.x; i < i1; i += 256) gw += e.grad[i] * e.param[i];
    return block_sum_256(gw, red);
}
// Step 2, any workgroup: one thread adds the tensor's partials in chunk order (chunks^2 serial loads per tensor when
// every workgroup of the tensor does it) and divides by sigma; broadcast through *c_lds.
__device__ __forceinline__ float tensor_sn_c(const calm_optim_tensor& e, const float* __restrict__ chunk_gw, float sg,
                                             float* c_lds) {
    if (threadIdx.x == 0) {
        const int nch = chunk_count(CHUNK_ELEMS, e.numel);
        float gw = 0.f;
        for (int k = 0; k < nch; ++k) gw += chunk_gw[e.chunk0 + k];        // fixed order: chunk 0, 1, 2, ...
        *c_lds = gw / sg;                                    // <G, W_orig / sigma>, as optim_finalize forms it
    }
    __syncthreads();
    return *c_lds;
}

// The loop of a kernel whose pointers come out of a table, so that the compiler cannot know that they do not alias and
// will not move a load across a store: a thread issues the loads of U accesses of W elements each ahead of the first
// store.  Over [i0, end), a span of at most one chunk with end - i0 a multiple of W (end <= i0: nothing); load(i) returns
// what the access at element i read (any type), store(i, v) consumes it.  NT = threads of the workgroup.  The position
// inside the span is an int: with 64-bit positions snapshot_move needs 28 VGPRs instead of 26, this way 24.
template <int U, int W, int NT, class Load, class Store>
__device__ __forceinline__ void loads_ahead_of_stores(long i0, long end, Load load, Store store) {
    const int n = end > i0 ? (int)(end - i0) : 0;
    for (int b = W * threadIdx.x; b < n; b += W * NT * U) {
        decltype(load(i0)) v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int o = b + u * W * NT;
            if (o < n) v[u] = load(i0 + o);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int o = b + u * W * NT;
            if (o < n) store(i0 + o, v[u]);
        }
    }
}
