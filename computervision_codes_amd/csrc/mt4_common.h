// Shared helpers for the gfx950 kernels of libmt4hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/mt4hip.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;

extern thread_local int g_mt4_last_hip_error;

// hipGetLastError() reports (and clears) the last error of ANY runtime call on this thread, including ones
// the host framework made earlier; clear it before a launch so that the check sees only our launch.
static inline void mt4_clear_error() { (void)hipGetLastError(); }

static inline int mt4_check_launch() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        g_mt4_last_hip_error = (int)e;
        return MT4_ELAUNCH;
    }
    return MT4_OK;
}

__device__ __forceinline__ float bf16_to_f32(u16 v) { return __uint_as_float(((uint32_t)v) << 16); }

// f32 -> bf16, round-to-nearest-even: a plain cast, which hipcc lowers to the gfx950 hardware convert
// (v_cvt_pk_bf16_f32, NaN stays NaN) -- an integer-arithmetic rounding costs ~6 VALU ops per element and made the
// conv epilogue VALU-issue-bound (SQ_ACTIVE_INST_ANY 41 % of wave cycles on the K=64 layers).
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16 f32_to_bf16(float f) {
    const __bf16 b = (__bf16)f;
    return __builtin_bit_cast(u16, b);
}

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// GELU, erf form (nn.GELU default): x Phi(x), Phi(x) = 0.5 erfc(-x / sqrt 2).  With a = min(|x|, 6) and Q(a) = -log2(erfc(a / sqrt 2)) fitted by
// a (c1 + a (c2 + a (c3 + a (c4 + a c5)))) (weighted least squares on the GELU error over [0, 6]):  t = 2^-Q(a) = erfc(a / sqrt 2),
//     gelu(x) = 0.5 x (1 + sign(x) (1 - t));      measured |gelu - exact| < 9e-7 over [-10, 10] in fp32 arithmetic.
// One transcendental (v_exp_f32) and 9 fma / mul / min / bfi per element, all of which pair up in the packed form below (v_pk_fma_f32 ...):
// 10 issue slots per element against 19 for the Abramowitz-Stegun 7.1.26 form of rounds 1-3 (1 rcp + 1 exp + 11 plain, no packing) and
// ~45 for libm's erff -- the fc1 (+ GELU) epilogues of Swin are VALU-bound on it (73728 x 2048 elements per launch at batch 128).
typedef float mt4_f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ mt4_f32x2 gelu_erf2(mt4_f32x2 x) {
    const mt4_f32x2 a = {fminf(fabsf(x.x), 6.0f), fminf(fabsf(x.y), 6.0f)};
    mt4_f32x2 p = a * 4.881283152809e-04f + -7.198873334067e-03f;
    p = p * a + 5.214694370026e-02f;
    p = p * a + 4.595955966962e-01f;
    p = p * a + 1.151000605814e+00f;
    const mt4_f32x2 q = p * a;
    const mt4_f32x2 t = {__builtin_amdgcn_exp2f(-q.x), __builtin_amdgcn_exp2f(-q.y)};
    const mt4_f32x2 u = 1.0f - t;
    const mt4_f32x2 hx = x * 0.5f;
    const mt4_f32x2 s = {__builtin_copysignf(u.x, x.x), __builtin_copysignf(u.y, x.y)};
    return hx * s + hx;
}
__device__ __forceinline__ float gelu_erf(float x) {      // (the same arithmetic on one value: identical results)
    const float a = fminf(fabsf(x), 6.0f);
    float p = fmaf(a, 4.881283152809e-04f, -7.198873334067e-03f);
    p = fmaf(p, a, 5.214694370026e-02f);
    p = fmaf(p, a, 4.595955966962e-01f);
    p = fmaf(p, a, 1.151000605814e+00f);
    const float t = __builtin_amdgcn_exp2f(-(p * a));
    const float hx = 0.5f * x;
    return fmaf(hx, __builtin_copysignf(1.0f - t, x), hx);
}
template <int N>
__device__ __forceinline__ void gelu_erf_n(float (&v)[N]) {
    static_assert(N % 2 == 0, "pairs");
#pragma unroll
    for (int e = 0; e < N; e += 2) {
        const mt4_f32x2 r = gelu_erf2((mt4_f32x2){v[e], v[e + 1]});
        v[e] = r.x; v[e + 1] = r.y;
    }
}

static inline int cdiv(int a, int b) { return (a + b - 1) / b; }

// Launch kernel `Fn` and report the launch's error.  A launch that needs more than 64 KiB of dynamic LDS first raises the kernel's limit on
// the CURRENT device, once per kernel and device: the attribute belongs to the kernel FUNCTION and the device, so the flag is keyed on the
// function itself (a non-type template parameter: a helper templated on the function's TYPE would share one flag among all kernels of one
// signature -- every igemm_conv_kernel<...> is void(ConvK) -- and a process-wide flag would leave a second GPU at the 64 KiB default)
template <auto Fn, typename... Args>
static inline int mt4_launch(dim3 grid, dim3 block, int lds, hipStream_t stream, const Args&... args) {
    if (lds > 65536) {
        static bool raised[64] = {};
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 64 || !raised[dev]) {
            (void)hipFuncSetAttribute((const void*)Fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (dev >= 0 && dev < 64) raised[dev] = true;
        }
    }
    hipLaunchKernelGGL(Fn, grid, block, lds, stream, args...);
    return mt4_check_launch();
}

// output / residual rows are stored / loaded with the non-temporal bit when the launch's output exceeds this many MB (below it the map fits the
// Infinity Cache and stays cacheable for the next layer; each byte is touched once per launch: +2.6 % frames/s on ResNet-50, +4.5 % on Swin-B,
// same-box A/Bs of round 1)
#define MT4_NT_MIN_MB 200

// ------------------------------------------------------------------------------------------------ device helpers shared between the sources
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef unsigned v4u __attribute__((ext_vector_type(4)));

// raw buffer descriptor (stride 0, num_records = bytes, gfx9 data-format word) from wave-uniform values
__device__ __forceinline__ v4u make_srd(const void* p, unsigned bytes) {
    const unsigned long long u = (unsigned long long)p;
    v4u r;
    r.x = __builtin_amdgcn_readfirstlane((unsigned)u);
    r.y = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32) & 0xffffu);
    r.z = __builtin_amdgcn_readfirstlane(bytes);
    r.w = 0x00020000u;
    return r;
}

// N LDS-DMA pieces in ONE asm statement (one M0 save/restore): piece i goes to LDS [lds_addr + i*STRIDE + lane*16) from
// buffer offset voff[i] (per lane, range-checked: out-of-range lanes write zeros) + soff (wave-uniform, NOT range-checked).
// STRIDE = bytes one staging pass of the whole workgroup covers (waves * 8 rows * 128 B).
// M0 (the DMA's LDS base) is compiler-reserved: saved, set and restored inside the statement.
template <int N, int STRIDE>
__device__ __forceinline__ void lds_dma16_group(v4u srd, const unsigned (&voff)[N], unsigned soff, unsigned lds_addr) {
    unsigned keep;
    if constexpr (N == 1) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff[0]), "s"(srd), "s"(soff), "s"(lds_addr) : "memory");
    } else if constexpr (N == 2) {
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %5\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %3, %4 offen lds\n\t"
                     "s_add_u32 m0, m0, %6\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %3, %4 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff[0]), "v"(voff[1]), "s"(srd), "s"(soff), "s"(lds_addr), "n"(STRIDE) : "memory", "scc");
    } else {
        static_assert(N == 4, "1, 2 or 4 pieces");
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %7\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %5, %6 offen lds\n\t"
                     "s_add_u32 m0, m0, %8\n\ts_nop 0\n\tbuffer_load_dwordx4 %2, %5, %6 offen lds\n\t"
                     "s_add_u32 m0, m0, %8\n\ts_nop 0\n\tbuffer_load_dwordx4 %3, %5, %6 offen lds\n\t"
                     "s_add_u32 m0, m0, %8\n\ts_nop 0\n\tbuffer_load_dwordx4 %4, %5, %6 offen lds\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(voff[0]), "v"(voff[1]), "v"(voff[2]), "v"(voff[3]), "s"(srd), "s"(soff), "s"(lds_addr),
                       "n"(STRIDE)
                     : "memory", "scc");
    }
}

// one LDS-DMA piece: 64 lanes x 16 B from buffer offset `voff` (per lane) to LDS [lds_addr + lane*16); out-of-range lanes write zeros
__device__ __forceinline__ void lds_dma16(v4u srd, unsigned voff, unsigned lds_addr) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %3\n\t"
        "s_nop 0\n\t"
        "buffer_load_dwordx4 %1, %2, 0 offen lds\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(srd), "s"(lds_addr)
        : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// 4 consecutive elements of a float or bf16 row as float4, and back (bf16: round to nearest even)
template <typename T> __device__ __forceinline__ float4 ld4(const T* p);
template <> __device__ __forceinline__ float4 ld4<float>(const float* p) { return *(const float4*)p; }
template <> __device__ __forceinline__ float4 ld4<u16>(const u16* p) {
    const uint2 v = *(const uint2*)p;
    return make_float4(__uint_as_float(v.x << 16), __uint_as_float(v.x & 0xffff0000u), __uint_as_float(v.y << 16), __uint_as_float(v.y & 0xffff0000u));
}
template <typename T> __device__ __forceinline__ void st4(T* p, float4 v);
template <> __device__ __forceinline__ void st4<float>(float* p, float4 v) { *(float4*)p = v; }
template <> __device__ __forceinline__ void st4<u16>(u16* p, float4 v) { *(uint2*)p = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the counter generator of every random draw (computervision_codes_amd/synth.py:uniform01 is the same function on the host side of the tests)
__host__ __device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
    x += 0x9E3779B97F4A7C15ULL;
    unsigned long long z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// ------------------------------------------------------------------------------------------------ train-mode BatchNorm: the reduction both tensor types share
// A thread owns 4 consecutive channels (one 16- or 8-byte load per row) and walks rows; the reductions run 1024-thread workgroups (64 channels
// x 64 row phases), at most ~512 per launch: every workgroup ends in 128 float64 atomics on its slab's 128 addresses, and 2048 workgroups of
// 256 threads on a 64-channel map made those same-address chains (~25 ns a link at the L2) longer than the stream itself -- 52-58 us for 59 MB
// where the apply kernel moves twice the bytes in 20-29 us (profiles/r03_bn_training_kernels.txt)
// DET (the `_det` entry points): `sums` is the workspace and row slab blockIdx.y STORES its 2 x C values into part blockIdx.y = sums + blockIdx.y * 2 C
// -- every channel of both rows, no atomics; mt4_fold_parts_f64 adds the slabs in index order afterwards
template <bool DET = false>
__device__ __forceinline__ void bn_block_reduce(double (&acc)[8], double* __restrict__ sums, int C, int c0) {
    __shared__ double red[16][8][17];               // [wave][value][channel group], padded
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 8; ++j) {                   // the 4 row phases of a wave
        acc[j] += __shfl_xor(acc[j], 16);
        acc[j] += __shfl_xor(acc[j], 32);
    }
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 8; ++j) red[w][j][lane] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x < 128) {                        // 16 channel groups x 8 values
        const int g = threadIdx.x & 15, j = threadIdx.x >> 4;
        double t = 0.0;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) t += red[rr][j][g];
        const int c = c0 + g * 4 + (j & 3);
        if constexpr (DET) {
            if (c < C) sums[(long long)blockIdx.y * 2 * C + (j >> 2) * C + c] = t;
        } else {
            if (c < C) atomicAdd(sums + (j >> 2) * C + c, t);
        }
    }
}

static inline int bn_reduce_slabs(long long M, int C) {                      // 64-row slabs of the 1024-thread reductions
    long long gy = (M + 63) / 64;
    const long long cap = (512 + cdiv(C, 64) - 1) / cdiv(C, 64);
    if (gy > cap) gy = cap;
    return gy < 1 ? 1 : (int)gy;
}

static inline int bn_row_slabs(long long M, int C) {                         // 16-row slabs of the 256-thread streaming kernels
    long long gy = (M + 63) / 64;
    const long long cap = (2048 + cdiv(C, 64) - 1) / cdiv(C, 64);
    if (gy > cap) gy = cap;
    return gy < 1 ? 1 : (int)gy;
}
