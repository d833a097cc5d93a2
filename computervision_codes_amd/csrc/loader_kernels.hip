// The sample rows of a training batch gathered on the device (loader.SampleTables): the label rows and the teacher prediction / feature rows
// the reference's dataset assembles per sample on the host (Spatial_cnn/dataloader.py:216-261) live in fp32 tables that are uploaded once per
// run; a batch (or a chunk of batches) is ONE launch over all tables.
#include <type_traits>

#include "mt4_common.h"

namespace {

struct TakeArgs {                       // passed BY VALUE in the kernel arguments (16 x 24 + 8 bytes): no descriptor upload, nothing to keep alive
    mt4_take_seg seg[MT4_TAKE_MAX_SEGS];
};

constexpr int TAKE_ROWS_PER_BLOCK = 8;  // 8 rows x 1536 floats = 12 float4 per thread; a grid of n / 8 x nseg workgroups (1280 for 1024 rows, 10 tables)

// blockIdx.y = segment, blockIdx.x = group of TAKE_ROWS_PER_BLOCK output rows.  VEC: C % 4 == 0 and both pointers 16-byte aligned -> every row starts
// on a 16-byte boundary, one dwordx4 load + store per element; otherwise dword accesses (C = 6, 10, 15: rows of 24 / 40 / 60 bytes).
// A row index outside [0, nrows) writes a zero row and reads nothing (the callers check on the host; this only keeps a bad index inside memory).
template <bool VEC>
__device__ __forceinline__ void take_rows_segment(const mt4_take_seg& sg, const long long* __restrict__ rows, long long r0, int nr) {
    typedef typename std::conditional<VEC, f32x4, float>::type T;
    const int W = VEC ? (sg.C >> 2) : sg.C;          // elements of T per row
    const T* __restrict__ src = (const T*)sg.table;
    T* __restrict__ dst = (T*)sg.out;
    const int total = nr * W;                        // <= 8 * C, C < 2^27 (checked by the entry point)
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        const int r = i / W, c = i - r * W;
        const long long s = rows[r0 + r];
        T v = {};
        if (s >= 0 && s < sg.nrows) v = src[s * W + c];
        dst[(r0 + r) * W + c] = v;
    }
}

__global__ __launch_bounds__(256) void take_rows_kernel(const TakeArgs a, const long long* __restrict__ rows, long long n) {
    const mt4_take_seg& sg = a.seg[blockIdx.y];
    const long long r0 = (long long)blockIdx.x * TAKE_ROWS_PER_BLOCK;
    const int nr = (int)((n - r0) < TAKE_ROWS_PER_BLOCK ? (n - r0) : TAKE_ROWS_PER_BLOCK);
    const bool vec = !(sg.C & 3) && !(((uintptr_t)sg.table | (uintptr_t)sg.out) & 15);      // (uniform over the workgroup)
    if (vec)
        take_rows_segment<true>(sg, rows, r0, nr);
    else
        take_rows_segment<false>(sg, rows, r0, nr);
}

}  // namespace

extern "C" int mt4_take_rows_f32(const mt4_take_seg* segs, int32_t nseg, const int64_t* rows, int64_t n, void* stream) {
    mt4_clear_error();
    if (!segs || nseg < 1 || nseg > MT4_TAKE_MAX_SEGS || n < 0) return MT4_EINVAL;
    TakeArgs a = {};
    for (int s = 0; s < nseg; ++s) {
        if (!segs[s].table || segs[s].C < 1 || segs[s].C >= (1 << 27) || segs[s].nrows < 1 || (n > 0 && !segs[s].out)) return MT4_EINVAL;
        if (((uintptr_t)segs[s].table | (uintptr_t)segs[s].out) & 3) return MT4_EALIGN;
        a.seg[s] = segs[s];
    }
    if (n == 0) return MT4_OK;                       // nothing to gather: no launch
    if (!rows) return MT4_EINVAL;
    const long long groups = (n + TAKE_ROWS_PER_BLOCK - 1) / TAKE_ROWS_PER_BLOCK;
    if (groups > 0x7fffffffLL) return MT4_EUNSUPPORTED;
    hipLaunchKernelGGL(take_rows_kernel, dim3((unsigned)groups, (unsigned)nseg), dim3(256), 0, (hipStream_t)stream, a, (const long long*)rows,
                       (long long)n);
    return mt4_check_launch();
}
