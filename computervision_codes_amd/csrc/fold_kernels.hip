// The fixed-order fold behind every deterministic (`_det`) entry point: a producing launch STORES one partial per workgroup slot into a
// caller-provided workspace (plain vector stores, no atomics, no tickets, nothing waits for another workgroup), and this launch, next on the
// stream, adds the slots in index order.  The sum of an element then depends on the launch geometry alone -- which the host-only plan queries
// (`mt4_*_det_plan`) give as a function of the shape -- and never on the order in which workgroups finish.
#include "mt4_common.h"

// V consecutive elements of one part, moved as one access (16 bytes in the vector forms)
template <typename T, int V>
struct alignas(sizeof(T) * V) fold_vec {
    T v[V];
};

// dst[i] = (accumulate ? dst[i] : 0) + (((parts[0][i] + parts[1][i]) + parts[2][i]) + ...): a thread owns V consecutive elements and walks the parts
// front to back, four part loads in flight ahead of their four adds (the launch is HBM-bound: it reads nparts x n elements once, there is no reuse)
template <typename T, int V>
__global__ __launch_bounds__(256) void fold_parts_kernel(const T* __restrict__ parts, int nparts, long long n, long long stride, T* __restrict__ dst,
                                                         int accumulate) {
    typedef fold_vec<T, V> vec;
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= n) return;                                     // (vector forms: n % V == 0, so a thread's V elements are all inside)
    const T* p = parts + i;
    vec t = *(const vec*)p;
    int q = 1;
    for (; q + 4 <= nparts; q += 4) {
        const vec a = *(const vec*)(p + (long long)q * stride), b = *(const vec*)(p + (long long)(q + 1) * stride);
        const vec c = *(const vec*)(p + (long long)(q + 2) * stride), d = *(const vec*)(p + (long long)(q + 3) * stride);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            t.v[e] += a.v[e];
            t.v[e] += b.v[e];
            t.v[e] += c.v[e];
            t.v[e] += d.v[e];
        }
    }
    for (; q < nparts; ++q) {
        const vec a = *(const vec*)(p + (long long)q * stride);
#pragma unroll
        for (int e = 0; e < V; ++e) t.v[e] += a.v[e];
    }
    if (accumulate) {
        const vec o = *(const vec*)(dst + i);
#pragma unroll
        for (int e = 0; e < V; ++e) t.v[e] = o.v[e] + t.v[e];
    }
    *(vec*)(dst + i) = t;
}

// Many parts of few elements (the BatchNorm slabs: up to 512 parts of 2 C float64; the scalar losses: a part element per workgroup): one thread per element
// would walk hundreds of dependent loads.  The parts are grouped into MT4_FOLD_CHUNKS = 16 chunks of L = ceil(nparts / 16) consecutive parts; a workgroup
// owns 16 elements, thread (chunk c, element e) adds chunk c's parts [c L, min((c + 1) L, nparts)) front to back, and the chunks that hold parts are then
// added front to back.  A fixed order, a function of nparts alone; nparts <= 16 makes it the plain sequential fold.
template <typename T>
__global__ __launch_bounds__(256) void fold_parts_chunked_kernel(const T* __restrict__ parts, int nparts, long long n, long long stride, T* __restrict__ dst,
                                                                 int accumulate, int L) {
    __shared__ T red[MT4_FOLD_CHUNKS][17];
    const int e = threadIdx.x & 15, c = threadIdx.x >> 4;
    const long long i = (long long)blockIdx.x * 16 + e;
    const int p0 = c * L, p1 = min(nparts, p0 + L);
    T t = 0;
    if (i < n && p0 < p1) {
        const T* p = parts + i;
        t = p[(long long)p0 * stride];
        int q = p0 + 1;
        for (; q + 4 <= p1; q += 4) {
            const T a = p[(long long)q * stride], b = p[(long long)(q + 1) * stride], c2 = p[(long long)(q + 2) * stride], d = p[(long long)(q + 3) * stride];
            t += a;
            t += b;
            t += c2;
            t += d;
        }
        for (; q < p1; ++q) t += p[(long long)q * stride];
    }
    red[c][e] = t;
    __syncthreads();
    if (c == 0 && i < n) {
        const int nch = (nparts + L - 1) / L;               // the chunks that hold parts
        T s = red[0][e];
        for (int k = 1; k < nch; ++k) s += red[k][e];
        dst[i] = accumulate ? dst[i] + s : s;
    }
}

template <typename T>
static int fold_parts_chunked(const T* parts, int32_t nparts, int64_t n, int64_t part_stride, T* dst, int32_t accumulate, void* stream) {
    mt4_clear_error();
    if (!parts || !dst || nparts <= 0 || n <= 0 || part_stride < n) return MT4_EINVAL;
    if (((uintptr_t)parts | (uintptr_t)dst) & (sizeof(T) - 1)) return MT4_EALIGN;
    const int L = (nparts + MT4_FOLD_CHUNKS - 1) / MT4_FOLD_CHUNKS;
    hipLaunchKernelGGL(fold_parts_chunked_kernel<T>, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, (hipStream_t)stream, parts, nparts, (long long)n,
                       (long long)part_stride, dst, accumulate, L);
    return mt4_check_launch();
}

template <typename T>
static int fold_parts(const T* parts, int32_t nparts, int64_t n, int64_t part_stride, T* dst, int32_t accumulate, void* stream) {
    mt4_clear_error();
    if (!parts || !dst || nparts <= 0 || n <= 0 || part_stride < n) return MT4_EINVAL;
    if (((uintptr_t)parts | (uintptr_t)dst) & (sizeof(T) - 1)) return MT4_EALIGN;
    constexpr int V = 16 / sizeof(T);
    hipStream_t s = (hipStream_t)stream;
    // 16-byte accesses where every part row and dst allow them; element accesses otherwise (bias slices, odd column counts: small folds)
    const bool wide = !(((uintptr_t)parts | (uintptr_t)dst) & 15) && part_stride % V == 0 && n % V == 0;
    if (wide) {
        const long long threads = n / V;
        hipLaunchKernelGGL((fold_parts_kernel<T, V>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, parts, nparts, (long long)n,
                           (long long)part_stride, dst, accumulate);
    } else {
        hipLaunchKernelGGL((fold_parts_kernel<T, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, parts, nparts, (long long)n,
                           (long long)part_stride, dst, accumulate);
    }
    return mt4_check_launch();
}

extern "C" int mt4_fold_parts_f32(const float* parts, int32_t nparts, int64_t n, int64_t part_stride, float* dst, int32_t accumulate, void* stream) {
    return fold_parts<float>(parts, nparts, n, part_stride, dst, accumulate, stream);
}

extern "C" int mt4_fold_parts_f64(const double* parts, int32_t nparts, int64_t n, int64_t part_stride, double* dst, int32_t accumulate, void* stream) {
    return fold_parts<double>(parts, nparts, n, part_stride, dst, accumulate, stream);
}

extern "C" int mt4_fold_parts_chunked_f32(const float* parts, int32_t nparts, int64_t n, int64_t part_stride, float* dst, int32_t accumulate, void* stream) {
    return fold_parts_chunked<float>(parts, nparts, n, part_stride, dst, accumulate, stream);
}

extern "C" int mt4_fold_parts_chunked_f64(const double* parts, int32_t nparts, int64_t n, int64_t part_stride, double* dst, int32_t accumulate, void* stream) {
    return fold_parts_chunked<double>(parts, nparts, n, part_stride, dst, accumulate, stream);
}
