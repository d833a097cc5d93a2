// The random pieces of a Temporal_tenco training step drawn on the device (`Temporal_tenco/network.py:43-48,123-127,194-196`): per-layer
// nn.Dropout fused into the residual add, the 75 % input mask with an EXACT count of ones, Dropout2d per input channel.
//
// Every draw is a function of a device-resident {seed, step} pair and a by-value slot:
//     base = splitmix64(seed * 0x100000001B3 + step * 4096 + slot),   key_i = splitmix64(base + i)
// -- `synth.uniform01(seed, step * 4096 + slot, n)` on the host.  Nothing of the draw is a kernel argument that a captured hipGraph would
// freeze: a replay sees a new draw when the host copies a new {seed, step} into the graph's static input.  A mask is never stored: the
// backward regenerates it from the same counters.
//
// Cost: a key is two 64 x 64 -> 64 bit multiplies (4 quarter-rate 32-bit multiplies each) and a few shifts / xors; at T = 2000 a step draws
// 42 M keys for the layer masks (twice: forward and backward) and 10 x 1 M for the select, tens of microseconds of VALU time on 256 CUs next
// to the 16-byte loads and stores the fused multiply needs anyway.
#include "mt4_common.h"

namespace {

// (uniform over the grid: the two loads are scalar loads, the finaliser runs once per wave)
__device__ __forceinline__ unsigned long long draw_base(const long long* __restrict__ state, int slot) {
    const unsigned long long seed = (unsigned long long)state[0], step = (unsigned long long)state[1];
    return splitmix64(seed * 0x100000001B3ULL + step * 4096ULL + (unsigned long long)slot);
}

// ------------------------------------------------------------------------------------------------ nn.Dropout fused into a multiply(-add)
// u_i >= p with u_i = (key_i >> 11) * 2^-53 (the comparison `dropout_mask_kernel` makes in double) is the integer comparison
// (key_i >> 11) >= ceil(p * 2^53): both sides scale exactly by 2^53.  `thr53` is that integer.
__global__ __launch_bounds__(256) void dropout_mul_add_kernel(const float* a, const float* c, float* y, long long n4,
                                                              const long long* __restrict__ state, int slot, unsigned long long thr53, float keep) {
    const long long i4 = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i4 >= n4) return;
    const unsigned long long b = draw_base(state, slot) + 4ULL * (unsigned long long)i4;
    const float4 av = ((const float4*)a)[i4];
    const float m0 = (splitmix64(b) >> 11) >= thr53 ? keep : 0.f;
    const float m1 = (splitmix64(b + 1) >> 11) >= thr53 ? keep : 0.f;
    const float m2 = (splitmix64(b + 2) >> 11) >= thr53 ? keep : 0.f;
    const float m3 = (splitmix64(b + 3) >> 11) >= thr53 ? keep : 0.f;
    float4 r;
    if (c) {
        const float4 cv = ((const float4*)c)[i4];
        r.x = fmaf(av.x, m0, cv.x); r.y = fmaf(av.y, m1, cv.y); r.z = fmaf(av.z, m2, cv.z); r.w = fmaf(av.w, m3, cv.w);
    } else {
        r.x = av.x * m0; r.y = av.y * m1; r.z = av.z * m2; r.w = av.w * m3;
    }
    ((float4*)y)[i4] = r;
}

// ------------------------------------------------------------------------------------------------ k-th smallest key: radix select
// 8 passes over the 64-bit keys, most significant byte first.  Pass p counts, among the keys whose p leading bytes equal the prefix found so
// far, the values of byte p: a 256-bin histogram per workgroup in LDS (after pass 0 one key in 256 still matches, so the LDS adds are few),
// added to the pass's bins in `scratch` with one global add per non-empty bin and workgroup.  The step from one pass to the next -- the byte
// at which the running count reaches the remaining k -- is taken redundantly by EVERY workgroup of the next pass from the previous pass's
// complete bins (a kernel boundary lies between them), so no workgroup waits for another and no ticket or fence is needed.  Keys are
// regenerated in every pass and never stored.
//
// scratch: unsigned hist[8][256], then unsigned long long st[9][2] = {prefix, remaining k} in front of pass p (st[0] from the clear kernel).
constexpr int SEL_PASSES = 8;
constexpr int SEL_ST_OFF = SEL_PASSES * 256 * 4;          // byte offset of st[] in scratch

__global__ __launch_bounds__(256) void select_clear_kernel(unsigned* __restrict__ hist, unsigned long long* __restrict__ st, unsigned long long k) {
    for (int i = threadIdx.x; i < SEL_PASSES * 256; i += 256) hist[i] = 0u;
    if (threadIdx.x == 0) { st[0] = 0ULL; st[1] = k; }
}

// {prefix, k} in front of pass p (>= 1) from the pair in front of pass p - 1 and that pass's bins; the same values in every thread of the block.
// With 1 <= k <= (sum of the bins) exactly one bin satisfies `below < k <= below + count`; with k == 0 none does and the prefix stays 0.
__device__ __forceinline__ void select_advance(const unsigned* __restrict__ hist, const unsigned long long* __restrict__ st, int p,
                                               unsigned long long& prefix, unsigned long long& krem) {
    __shared__ unsigned sc[256];
    __shared__ unsigned long long s_next[2];
    const int tid = threadIdx.x;
    const unsigned long long prefix0 = st[2 * (p - 1)], k0 = st[2 * (p - 1) + 1];
    const unsigned cnt = hist[(p - 1) * 256 + tid];
    sc[tid] = cnt;
    if (tid == 0) { s_next[0] = prefix0; s_next[1] = 0ULL; }
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {             // inclusive scan of the 256 bins
        const unsigned v = tid >= off ? sc[tid - off] : 0u;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    const unsigned long long incl = sc[tid], below = incl - cnt;
    if (below < k0 && k0 <= incl) {
        s_next[0] = prefix0 | ((unsigned long long)tid << (56 - 8 * (p - 1)));
        s_next[1] = k0 - below;
    }
    __syncthreads();
    prefix = s_next[0];
    krem = s_next[1];
}

__global__ __launch_bounds__(256) void select_pass_kernel(long long n, const long long* __restrict__ state, int slot, unsigned* __restrict__ hist,
                                                          unsigned long long* __restrict__ st, int p) {
    __shared__ unsigned h[256];
    const int tid = threadIdx.x;
    unsigned long long prefix = 0ULL, krem = 0ULL;
    if (p > 0) {
        select_advance(hist, st, p, prefix, krem);
        if (blockIdx.x == 0 && tid == 0) { st[2 * p] = prefix; st[2 * p + 1] = krem; }
    }
    h[tid] = 0u;
    __syncthreads();
    const unsigned long long base = draw_base(state, slot);
    const unsigned long long himask = p == 0 ? 0ULL : ~0ULL << (64 - 8 * p);
    const int shift = 56 - 8 * p;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n; i += stride) {
        const unsigned long long key = splitmix64(base + (unsigned long long)i);
        if ((key & himask) == prefix) atomicAdd(&h[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (h[tid]) atomicAdd(&hist[p * 256 + tid], h[tid]);
}

__global__ __launch_bounds__(256) void select_finish_kernel(const unsigned* __restrict__ hist, const unsigned long long* __restrict__ st,
                                                            unsigned long long* __restrict__ thr) {
    unsigned long long prefix, krem;
    select_advance(hist, st, SEL_PASSES, prefix, krem);
    if (threadIdx.x == 0) *thr = prefix;
}

// ------------------------------------------------------------------------------------------------ input mask + Dropout2d
// y[t][d] = x[t][d] * (key(t*D + d) <= *thr ? 1 : 0) * (u_chan(d) >= 0.5 ? 2 : 0); four consecutive d per thread (D % 4 == 0: one row)
__global__ __launch_bounds__(256) void tenco_input_draw_kernel(const float* x, float* y, unsigned n4, unsigned D, const long long* __restrict__ state,
                                                               int slot_keys, const unsigned long long* __restrict__ thr, int slot_chan) {
    const unsigned i4 = blockIdx.x * 256u + threadIdx.x;
    if (i4 >= n4) return;
    const unsigned i = 4u * i4, d = i % D;
    const unsigned long long bc = draw_base(state, slot_chan) + d;
    const unsigned long long half = 1ULL << 52;           // u >= 0.5  <=>  (key >> 11) >= 2^52
    float4 v = ((const float4*)x)[i4];
    if (thr) {
        const unsigned long long t = *thr, bk = draw_base(state, slot_keys) + i;
        v.x *= splitmix64(bk) <= t ? 1.f : 0.f;
        v.y *= splitmix64(bk + 1) <= t ? 1.f : 0.f;
        v.z *= splitmix64(bk + 2) <= t ? 1.f : 0.f;
        v.w *= splitmix64(bk + 3) <= t ? 1.f : 0.f;
    }
    v.x *= (splitmix64(bc) >> 11) >= half ? 2.f : 0.f;
    v.y *= (splitmix64(bc + 1) >> 11) >= half ? 2.f : 0.f;
    v.z *= (splitmix64(bc + 2) >> 11) >= half ? 2.f : 0.f;
    v.w *= (splitmix64(bc + 3) >> 11) >= half ? 2.f : 0.f;
    ((float4*)y)[i4] = v;
}

inline bool slot_ok(int32_t s) { return s >= 0 && s < 4096; }

}  // namespace

extern "C" int mt4_dropout_mul_add_f32(const float* a, const float* c, float* y, int64_t n, const int64_t* state, int32_t slot, float p, void* stream) {
    mt4_clear_error();
    if (!a || !y || !state || n <= 0 || (n & 3) || !slot_ok(slot) || !(p >= 0.f) || p >= 1.f) return MT4_EINVAL;
    if ((((uintptr_t)a | (uintptr_t)y | (uintptr_t)c) & 15) != 0) return MT4_EINVAL;
    const double scaled = (double)p * 9007199254740992.0;                  // exact: a power-of-two scaling of a float
    unsigned long long thr53 = (unsigned long long)scaled;
    if ((double)thr53 < scaled) ++thr53;                                   // ceil
    const long long n4 = n >> 2;
    hipLaunchKernelGGL(dropout_mul_add_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, c, y, n4,
                       (const long long*)state, (int)slot, thr53, 1.0f / (1.0f - p));
    return mt4_check_launch();
}

extern "C" int mt4_select_kth_key_u64(uint64_t* thr, int64_t n, int64_t k, const int64_t* state, int32_t slot, void* scratch, void* stream) {
    mt4_clear_error();
    if (!thr || !state || !scratch || n <= 0 || k < 0 || k > n || !slot_ok(slot)) return MT4_EINVAL;
    if ((((uintptr_t)thr | (uintptr_t)scratch) & 7) != 0) return MT4_EINVAL;
    if (n > 0x7FFFFFFFLL) return MT4_EUNSUPPORTED;                         // the bins are 32-bit counts
    static_assert(SEL_ST_OFF + (SEL_PASSES + 1) * 16 <= MT4_SELECT_SCRATCH_BYTES, "scratch layout");
    unsigned* hist = (unsigned*)scratch;
    unsigned long long* st = (unsigned long long*)((char*)scratch + SEL_ST_OFF);
    hipStream_t s = (hipStream_t)stream;
    long long blocks = (n + 2047) / 2048;                                   // >= 8 keys per thread and pass, at most one workgroup per CU
    if (blocks > 256) blocks = 256;
    hipLaunchKernelGGL(select_clear_kernel, dim3(1), dim3(256), 0, s, hist, st, (unsigned long long)k);
    for (int p = 0; p < SEL_PASSES; ++p)
        hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (long long)n, (const long long*)state, (int)slot, hist, st, p);
    hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(256), 0, s, (const unsigned*)hist, (const unsigned long long*)st, (unsigned long long*)thr);
    return mt4_check_launch();
}

extern "C" int mt4_tenco_input_draw_f32(const float* x, float* y, int32_t T, int32_t D, const int64_t* state, int32_t slot_keys, const uint64_t* thr,
                                        int32_t slot_chan, void* stream) {
    mt4_clear_error();
    if (!x || !y || !state || T <= 0 || D <= 0 || (D & 3) || !slot_ok(slot_keys) || !slot_ok(slot_chan)) return MT4_EINVAL;
    if ((((uintptr_t)x | (uintptr_t)y) & 15) != 0 || ((uintptr_t)thr & 7) != 0) return MT4_EINVAL;
    const long long n = (long long)T * D;
    if (n > 0x7FFFFFFFLL) return MT4_EUNSUPPORTED;
    const unsigned n4 = (unsigned)(n >> 2);
    hipLaunchKernelGGL(tenco_input_draw_kernel, dim3((n4 + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, x, y, n4, (unsigned)D,
                       (const long long*)state, (int)slot_keys, (const unsigned long long*)thr, (int)slot_chan);
    return mt4_check_launch();
}
