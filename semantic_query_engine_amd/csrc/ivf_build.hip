// ivf_build.hip -- the small kernels behind IVF training and list building, and their launchers (ivf_kernels.h): the row
// gather and the two k-means update kernels of ivf_train, the assignment stores of ivf_assign_rows / ivf_rows_updated, and
// the count and scatter passes of ivf_build_lists.  Called from ivf.hip only.
#include "ivf_kernels.h"

namespace sqe {

namespace {

__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ x, const int64_t* __restrict__ idx,
                                                          int n, int dim, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const float4* s = reinterpret_cast<const float4*>(x + (size_t)idx[r] * dim);
    float4* d = reinterpret_cast<float4*>(out + (size_t)r * dim);
    for (int v = lane; v < (dim >> 2); v += 64) d[v] = s[v];
}

// sums[assign[r]] += x[r] (fp32 atomics, 256 contiguous bytes per wave-instruction); counts[assign[r]]++
__global__ __launch_bounds__(256) void kmeans_accum_kernel(const float* __restrict__ x, const int64_t* __restrict__ assign,
                                                           int64_t n, int dim, float* __restrict__ sums,
                                                           int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int64_t a = assign[r];
    if (a < 0) return;
    const float* s = x + (size_t)r * dim;
    float* d = sums + (size_t)a * dim;
    for (int i = lane; i < dim; i += 64) atomicAdd(d + i, s[i]);
    if (lane == 0) atomicAdd(counts + a, 1);
}

// centroid = sums / ||sums|| where the list is non-empty; empty lists keep their old centroid
__global__ __launch_bounds__(256) void kmeans_finish_kernel(float* __restrict__ centroids, const float* __restrict__ sums,
                                                            const int* __restrict__ counts, int nlist, int dim) {
    const int lane = threadIdx.x & 63;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nlist || counts[c] == 0) return;
    const float* s = sums + (size_t)c * dim;
    float ss = 0.f;
    for (int i = lane; i < dim; i += 64) ss += s[i] * s[i];
    const float den = sqrtf(wave_sum(ss)) + 1e-9f;
    for (int i = lane; i < dim; i += 64) centroids[(size_t)c * dim + i] = s[i] / den;
}

__global__ void ivf_store_assign_kernel(const int64_t* __restrict__ ids, int64_t n, int* __restrict__ assign,
                                        int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int a = (int)ids[i];
    assign[i] = a;
    if (counts && a >= 0) atomicAdd(counts + a, 1);
}

// assign[rows[i]] = lists[i] (rows overwritten by sqe_index_update)
__global__ void ivf_scatter_assign_kernel(const int* __restrict__ lists, const int64_t* __restrict__ rows, int64_t n,
                                          int* __restrict__ assign) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) assign[rows[i]] = lists[i];
}

__global__ void ivf_count_kernel(const int* __restrict__ assign, int64_t n, int* __restrict__ counts) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && assign[i] >= 0) atomicAdd(counts + assign[i], 1);
}

// order[p] = the row at position p of the list-ordered sequence; dpos[p] = its row in the int8 copy, where every list starts
// on a 256-row tile (tile_off: tiles in front of each list)
__global__ void ivf_scatter_kernel(const int* __restrict__ assign, int64_t n, const int64_t* __restrict__ offsets,
                                   const int64_t* __restrict__ tile_off, int* __restrict__ cursor, int* __restrict__ order,
                                   int* __restrict__ dpos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int a = assign[i];
    if (a < 0) return;
    const int c = atomicAdd(cursor + a, 1);
    order[offsets[a] + c] = (int)i;
    dpos[offsets[a] + c] = (int)(tile_off[a] * 256 + c);
}

}  // namespace

int launch_gather_rows(const float* x, const int64_t* idx, int n, int dim, float* out, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, idx, n, dim, out);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_kmeans_accum(const float* x, const int64_t* assign, int64_t n, int dim, float* sums, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_accum_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, x, assign, n, dim, sums, counts);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_kmeans_finish(float* centroids, const float* sums, const int* counts, int nlist, int dim, hipStream_t s) {
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((nlist + 3) / 4), dim3(256), 0, s, centroids, sums, counts, nlist, dim);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_store_assign(const int64_t* ids, int64_t n, int* assign, hipStream_t s) {
    hipLaunchKernelGGL(ivf_store_assign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ids, n, assign, (int*)nullptr);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_scatter_assign(const int* lists, const int64_t* rows, int64_t n, int* assign, hipStream_t s) {
    hipLaunchKernelGGL(ivf_scatter_assign_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, lists, rows, n, assign);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_count(const int* assign, int64_t n, int* counts, hipStream_t s) {
    if (n <= 0) return SQE_OK;
    hipLaunchKernelGGL(ivf_count_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, assign, n, counts);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

int launch_ivf_scatter(const int* assign, int64_t n, const int64_t* offsets, const int64_t* tile_off, int* cursor, int* order, int* dpos,
                       hipStream_t s) {
    if (n <= 0) return SQE_OK;
    hipLaunchKernelGGL(ivf_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, assign, n, offsets, tile_off, cursor, order,
                       dpos);
    SQE_HIP(hipGetLastError());
    return SQE_OK;
}

}  // namespace sqe
