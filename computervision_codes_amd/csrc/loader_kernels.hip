// The sample rows of a training batch gathered on the device (loader.SampleTables): the label rows and the teacher prediction / feature rows
// the reference's dataset assembles per sample on the host (Spatial_cnn/dataloader.py:216-261) live in fp32 tables that are uploaded once per
// run; a batch (or a chunk of batches) is ONE launch over all tables.
// The frame pool of cholect.FrameCache (--frame_cache): resized uint8 frames kept in HBM across epochs; a chunk's stores into the pool and its reads
// from it are one launch each over (16-byte pieces, frame), rows picked by a slot list.
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

// ------------------------------------------------------------------------------------------------ the frame pool
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

constexpr int FRAME_PIECES_PER_THREAD = 4;                                  // 4 x 16 bytes loaded before the first store: 16 KiB in flight per workgroup,
constexpr int FRAME_PIECES_PER_BLOCK = 256 * FRAME_PIECES_PER_THREAD;       // 128 KiB per CU at 8 resident workgroups (a streaming CU needs ~32 KiB)

// blockIdx.y = frame i, blockIdx.x = group of 1024 16-byte pieces of its row.  PUT: pool[slots[i]] = frames[i], else frames[i] = pool[slots[i]].
// A row whose slot is negative or >= pool_slots is skipped by the whole workgroup (uniform): nothing of it is read or written.
// VEC: frame_bytes % 16 == 0 and both bases 16-byte aligned -> every row of either side starts on a 16-byte boundary.  The pool side is touched once
// per epoch (tens of GB between two uses): non-temporal on that side; the chunk side is written / read by the neighbouring kernels: cacheable.
// Offsets are 64-bit: slot * frame_bytes passes 2^31 at slot 6242 of a 256 x 448 pool.
template <bool PUT, bool VEC>
__global__ __launch_bounds__(256) void frames_copy_kernel(unsigned char* __restrict__ pool, const int* __restrict__ slots, unsigned char* __restrict__ frames,
                                                          long long frame_bytes, long long pool_slots) {
    const long long s = slots[blockIdx.y];
    if (s < 0 || s >= pool_slots) return;
    unsigned char* prow = pool + s * frame_bytes;
    unsigned char* frow = frames + (long long)blockIdx.y * frame_bytes;
    const unsigned char* __restrict__ src = PUT ? frow : prow;
    unsigned char* __restrict__ dst = PUT ? prow : frow;
    const long long p0 = (long long)blockIdx.x * FRAME_PIECES_PER_BLOCK + threadIdx.x;
    if constexpr (VEC) {
        const long long pieces = frame_bytes >> 4;
        u32x4_t v[FRAME_PIECES_PER_THREAD];
#pragma unroll
        for (int j = 0; j < FRAME_PIECES_PER_THREAD; ++j) {
            const long long p = p0 + j * 256;
            if (p < pieces) v[j] = PUT ? *((const u32x4_t*)src + p) : __builtin_nontemporal_load((const u32x4_t*)src + p);
        }
#pragma unroll
        for (int j = 0; j < FRAME_PIECES_PER_THREAD; ++j) {
            const long long p = p0 + j * 256;
            if (p < pieces) {
                if (PUT) __builtin_nontemporal_store(v[j], (u32x4_t*)dst + p);
                else *((u32x4_t*)dst + p) = v[j];
            }
        }
    } else {                                                                // any size, any alignment: byte by byte
        for (int j = 0; j < FRAME_PIECES_PER_THREAD; ++j) {
            const long long b0 = (p0 + j * 256) << 4;
            const long long b1 = b0 + 16 < frame_bytes ? b0 + 16 : frame_bytes;
            for (long long b = b0; b < b1; ++b) dst[b] = src[b];
        }
    }
}

template <bool PUT>
int frames_copy(const void* pool, const int32_t* slots, const void* frames, int32_t n, int64_t frame_bytes, int64_t pool_slots, void* stream) {
    mt4_clear_error();
    if (n < 0 || frame_bytes <= 0 || pool_slots <= 0) return MT4_EINVAL;
    if (n == 0) return MT4_OK;                       // nothing to move: no launch
    if (!pool || !slots || !frames) return MT4_EINVAL;
    if ((uintptr_t)slots & 3) return MT4_EALIGN;
    const long long groups = ((frame_bytes + 15) / 16 + FRAME_PIECES_PER_BLOCK - 1) / FRAME_PIECES_PER_BLOCK;
    if (n > 65535 || groups > 0x7fffffffLL) return MT4_EUNSUPPORTED;
    const bool vec = !(frame_bytes & 15) && !(((uintptr_t)pool | (uintptr_t)frames) & 15);
    const dim3 grid((unsigned)groups, (unsigned)n);
    if (vec)
        hipLaunchKernelGGL((frames_copy_kernel<PUT, true>), grid, dim3(256), 0, (hipStream_t)stream, (unsigned char*)pool, (const int*)slots,
                           (unsigned char*)frames, (long long)frame_bytes, (long long)pool_slots);
    else
        hipLaunchKernelGGL((frames_copy_kernel<PUT, false>), grid, dim3(256), 0, (hipStream_t)stream, (unsigned char*)pool, (const int*)slots,
                           (unsigned char*)frames, (long long)frame_bytes, (long long)pool_slots);
    return mt4_check_launch();
}

}  // namespace

extern "C" int mt4_put_frames_u8(void* pool, const int32_t* slots, const void* frames, int32_t n, int64_t frame_bytes, int64_t pool_slots, void* stream) {
    return frames_copy<true>(pool, slots, frames, n, frame_bytes, pool_slots, stream);
}

extern "C" int mt4_take_frames_u8(const void* pool, const int32_t* slots, void* frames, int32_t n, int64_t frame_bytes, int64_t pool_slots, void* stream) {
    return frames_copy<false>(pool, slots, frames, n, frame_bytes, pool_slots, stream);
}

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
