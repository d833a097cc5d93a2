// The guarded update of the flat-parameter trainers (--clip_grad_norm, --skip_nonfinite): one pass over the flat gradient G that STORES a float64 sum of
// squares and a count of non-finite elements per workgroup (no atomics: the mechanism of the `_det` entry points, csrc/fold_kernels.hip), a one-workgroup
// finalize that folds them in the fixed chunks of mt4_fold_parts_chunked_f64 and writes the clip coefficient and the skip decision into device memory, and
// the SGD update / the restore that read them there.  Nothing between the gradient and the update touches the host.
#include "mt4_common.h"

#define GN_THREADS 256
#define GN_PART_ELEMS 16384LL      // elements of G per workgroup: 16 float4 per lane, four loads in flight per lane

struct alignas(16) gn_part {
    double sumsq;
    long long nonfinite;
};

__device__ __forceinline__ int gn_nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// workgroup z: the part [z PART, min(n, (z + 1) PART)) of g.  HBM-bound (G is read once, nothing is reused): 16-byte loads, four per lane ahead of their
// adds.  A float's square is exact in double, so fma(x, x, a) and a + x * x are the same value: only the additions round.
__global__ __launch_bounds__(GN_THREADS) void grad_norm_parts_kernel(const float* __restrict__ g, long long n, gn_part* __restrict__ parts) {
    __shared__ double wsum[GN_THREADS / 64];
    __shared__ int wcnt[GN_THREADS / 64];
    const long long lo = (long long)blockIdx.x * GN_PART_ELEMS, hi = min(n, lo + GN_PART_ELEMS);
    const long long full = lo + (hi - lo) / 4 * 4;               // the float4s of the part that lie inside n (lo % 4 == 0)
    double a0 = 0., a1 = 0., a2 = 0., a3 = 0.;
    int cnt = 0;
    long long i = lo + (long long)threadIdx.x * 4;
    constexpr long long S = GN_THREADS * 4;
    for (; i + 3 * S + 3 < full; i += 4 * S) {
        const float4 v0 = *(const float4*)(g + i), v1 = *(const float4*)(g + i + S), v2 = *(const float4*)(g + i + 2 * S),
                     v3 = *(const float4*)(g + i + 3 * S);
#define GN_ACC(v)                                                                                                          \
    a0 += (double)v.x * (double)v.x; a1 += (double)v.y * (double)v.y; a2 += (double)v.z * (double)v.z; a3 += (double)v.w * (double)v.w; \
    cnt += gn_nonfinite(v.x) + gn_nonfinite(v.y) + gn_nonfinite(v.z) + gn_nonfinite(v.w);
        GN_ACC(v0) GN_ACC(v1) GN_ACC(v2) GN_ACC(v3)
    }
    for (; i + 3 < full; i += S) {
        const float4 v = *(const float4*)(g + i);
        GN_ACC(v)
    }
#undef GN_ACC
    if (i == full && full < hi) {                                // the last, partial float4 of G (n % 4 elements): the lane whose turn it is, element by element
        const float x = g[full], y = full + 1 < hi ? g[full + 1] : 0.f, z = full + 2 < hi ? g[full + 2] : 0.f;
        a0 += (double)x * (double)x; a1 += (double)y * (double)y; a2 += (double)z * (double)z;
        cnt += gn_nonfinite(x) + gn_nonfinite(y) + gn_nonfinite(z);
    }
    double s = ((a0 + a1) + a2) + a3;
    for (int o = 32; o > 0; o >>= 1) {
        s += __shfl_xor(s, o);
        cnt += __shfl_xor(cnt, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        wsum[w] = s;
        wcnt[w] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        gn_part p;
        p.sumsq = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        p.nonfinite = (long long)wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        parts[blockIdx.x] = p;                                   // one 16-byte vector store into the workgroup's own slot
    }
}

extern "C" int mt4_grad_norm_plan(int64_t n, int32_t* nparts, int64_t* part_elems, int64_t* ws_bytes) {
    if (n <= 0) return MT4_EINVAL;
    const int64_t np = (n + GN_PART_ELEMS - 1) / GN_PART_ELEMS;
    if (np > 0x7fffffffLL) return MT4_EINVAL;
    if (nparts) *nparts = (int32_t)np;
    if (part_elems) *part_elems = GN_PART_ELEMS;
    if (ws_bytes) *ws_bytes = np * (int64_t)sizeof(gn_part);
    return MT4_OK;
}

extern "C" int mt4_grad_norm_parts_f32(const float* g, int64_t n, void* parts, int64_t parts_bytes, void* stream) {
    mt4_clear_error();
    int32_t np = 0;
    int64_t need = 0;
    if (!g || !parts || mt4_grad_norm_plan(n, &np, nullptr, &need) != MT4_OK || parts_bytes < need) return MT4_EINVAL;
    if (((uintptr_t)g | (uintptr_t)parts) & 15) return MT4_EALIGN;
    hipLaunchKernelGGL(grad_norm_parts_kernel, dim3((unsigned)np), dim3(GN_THREADS), 0, (hipStream_t)stream, g, (long long)n, (gn_part*)parts);
    return mt4_check_launch();
}

// One workgroup.  sumsq: the order of fold_parts_chunked_kernel (csrc/fold_kernels.hip) -- MT4_FOLD_CHUNKS chunks of L = ceil(nparts / 16) consecutive
// parts, thread c adds chunk c front to back, thread 0 the chunks that hold parts front to back.  The counts are integers: any order.
__global__ __launch_bounds__(GN_THREADS) void grad_guard_finalize_kernel(const gn_part* __restrict__ parts, int nparts, int L, float grad_scale,
                                                                         double max_norm, int skip_nonfinite, mt4_guard_state* __restrict__ state,
                                                                         mt4_guard_stats* __restrict__ stats) {
    __shared__ double red[MT4_FOLD_CHUNKS];
    __shared__ long long cred[GN_THREADS];
    const int c = threadIdx.x;
    if (c < MT4_FOLD_CHUNKS) {
        const int p0 = c * L, p1 = min(nparts, p0 + L);
        double t = 0.;
        if (p0 < p1) {
            t = parts[p0].sumsq;
            int q = p0 + 1;
            for (; q + 4 <= p1; q += 4) {
                const double a = parts[q].sumsq, b = parts[q + 1].sumsq, c2 = parts[q + 2].sumsq, d = parts[q + 3].sumsq;
                t += a;
                t += b;
                t += c2;
                t += d;
            }
            for (; q < p1; ++q) t += parts[q].sumsq;
        }
        red[c] = t;
    }
    long long k = 0;
    for (int q = c; q < nparts; q += GN_THREADS) k += parts[q].nonfinite;
    cred[c] = k;
    __syncthreads();
    for (int o = GN_THREADS / 2; o > 0; o >>= 1) {
        if (c < o) cred[c] += cred[c + o];
        __syncthreads();
    }
    if (c != 0) return;
    const int nch = (nparts + L - 1) / L;                        // the chunks that hold parts
    double s = red[0];
    for (int j = 1; j < nch; ++j) s += red[j];
    const long long bad = cred[0];
    const double norm = fabs((double)grad_scale) * sqrt(s);
    float coef = 1.f;
    if (max_norm > 0. && bad == 0) {                             // (the clip is not evaluated on a non-finite norm)
        const double r = max_norm / (norm + 1e-6);
        if (r < 1.) coef = (float)r;
    }
    const int skip = skip_nonfinite && bad > 0;
    state->sumsq = s;
    state->norm = norm;
    state->coef = coef;
    state->skip = skip;
    state->nonfinite = bad;
    stats->steps += 1;
    if (skip) {
        stats->skipped += 1;
    } else {
        if (coef < 1.f) stats->clipped += 1;
        stats->norm_sum += norm;
        if (norm > stats->norm_max) stats->norm_max = norm;
    }
}

extern "C" int mt4_grad_guard_finalize(const void* parts, int32_t nparts, float grad_scale, double max_norm, int32_t skip_nonfinite,
                                       mt4_guard_state* state, mt4_guard_stats* stats, void* stream) {
    mt4_clear_error();
    if (!parts || !state || !stats || nparts <= 0 || !(max_norm >= 0.)) return MT4_EINVAL;
    if (((uintptr_t)parts & 15) || (((uintptr_t)state | (uintptr_t)stats) & 7)) return MT4_EALIGN;
    const int L = (nparts + MT4_FOLD_CHUNKS - 1) / MT4_FOLD_CHUNKS;
    hipLaunchKernelGGL(grad_guard_finalize_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, (const gn_part*)parts, nparts, L, grad_scale,
                       max_norm, skip_nonfinite ? 1 : 0, state, stats);
    return mt4_check_launch();
}

// the body of sgd_kernel (csrc/train_kernels.hip) with gscale * state->coef for gscale; a skipped step writes nothing
__global__ void sgd_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, long long n, float lr, float wd, float grad_scale,
                                   const mt4_guard_state* __restrict__ state) {
    if (state->skip) return;
    const float gscale = grad_scale * state->coef;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 pv = *(float4*)(p + i);
        const float4 gv = *(const float4*)(g + i);
        pv.x -= lr * (gv.x * gscale + wd * pv.x); pv.y -= lr * (gv.y * gscale + wd * pv.y);
        pv.z -= lr * (gv.z * gscale + wd * pv.z); pv.w -= lr * (gv.w * gscale + wd * pv.w);
        *(float4*)(p + i) = pv;
    } else {
        for (long long j = i; j < n; ++j) p[j] -= lr * (g[j] * gscale + wd * p[j]);
    }
}

extern "C" int mt4_sgd_step_guarded_f32(float* p, const float* g, int64_t n, float lr, float weight_decay, float grad_scale,
                                        const mt4_guard_state* state, void* stream) {
    mt4_clear_error();
    if (!p || !g || !state || n <= 0) return MT4_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g) & 15) || ((uintptr_t)state & 7)) return MT4_EALIGN;
    const long long threads = (n + 3) / 4;
    hipLaunchKernelGGL(sgd_guarded_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, (long long)n, lr,
                       weight_decay, grad_scale, state);
    return mt4_check_launch();
}

__global__ void restore_if_skipped_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n,
                                          const mt4_guard_state* __restrict__ state) {
    if (!state->skip) return;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        *(float4*)(dst + i) = *(const float4*)(src + i);
    } else {
        for (long long j = i; j < n; ++j) dst[j] = src[j];
    }
}

extern "C" int mt4_restore_if_skipped_f32(float* dst, const float* src, int64_t n, const mt4_guard_state* state, void* stream) {
    mt4_clear_error();
    if (!dst || !src || !state || n <= 0) return MT4_EINVAL;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) || ((uintptr_t)state & 7)) return MT4_EALIGN;
    const long long threads = (n + 3) / 4;
    hipLaunchKernelGGL(restore_if_skipped_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dst, src,
                       (long long)n, state);
    return mt4_check_launch();
}

// ------------------------------------------------------------------------------------------------ optimizer state (--momentum, --nesterov, --optimizer adamw)
// Elementwise over the flat fp32 buffers: 16-byte loads and stores, the n % 4 tail element by element in the thread whose float4 it would be.  Every
// operation below is ONE round-to-nearest IEEE operation in the order written (no FMA contraction: the pragma in each body), so that the numpy float32
// restatement `ops.optim_step_host` gives the same bits.  guard == NULL: unguarded (coef 1, never skipped).

// the step record of AdamW: advanced by one thread ahead of the update unless the guard says skip; IEEE double multiplies
__global__ void optim_advance_kernel(mt4_optim_state* __restrict__ os, double beta1, double beta2, const mt4_guard_state* __restrict__ guard) {
    if (guard && guard->skip) return;
    os->t += 1;
    os->beta1_pow *= beta1;
    os->beta2_pow *= beta2;
}

extern "C" int mt4_optim_advance(mt4_optim_state* optim_state, double beta1, double beta2, const mt4_guard_state* guard_state, void* stream) {
    mt4_clear_error();
    if (!optim_state || !(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.)) return MT4_EINVAL;
    if ((((uintptr_t)optim_state) | (uintptr_t)guard_state) & 7) return MT4_EINVAL;
    hipLaunchKernelGGL(optim_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, optim_state, beta1, beta2, guard_state);
    return mt4_check_launch();
}

// torch.optim.SGD(momentum, dampening 0, nesterov).  Per thread: s = grad_scale * coef (float).  Per element, all float:
//   d = g * s + wd * p;   m' = mom * m + d;   u = nesterov ? d + mom * m' : m';   p' = p - lr * u
__device__ __forceinline__ void sgdm_elem(float& p, float g, float& m, float lr, float wd, float s, float mom, int nesterov) {
#pragma clang fp contract(off)
    const float gs = g * s;
    const float wp = wd * p;
    const float d = gs + wp;
    const float mm = mom * m;
    const float mn = mm + d;
    float u = mn;
    if (nesterov) {
        const float t = mom * mn;
        u = d + t;
    }
    const float lu = lr * u;
    p = p - lu;
    m = mn;
}

__global__ void sgd_momentum_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, long long n, float lr, float wd,
                                    float grad_scale, float mom, int nesterov, const mt4_guard_state* __restrict__ guard) {
#pragma clang fp contract(off)
    if (guard && guard->skip) return;
    const float s = guard ? grad_scale * guard->coef : grad_scale;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 pv = *(float4*)(p + i), mv = *(float4*)(m + i);
        const float4 gv = *(const float4*)(g + i);
        sgdm_elem(pv.x, gv.x, mv.x, lr, wd, s, mom, nesterov); sgdm_elem(pv.y, gv.y, mv.y, lr, wd, s, mom, nesterov);
        sgdm_elem(pv.z, gv.z, mv.z, lr, wd, s, mom, nesterov); sgdm_elem(pv.w, gv.w, mv.w, lr, wd, s, mom, nesterov);
        *(float4*)(p + i) = pv;
        *(float4*)(m + i) = mv;
    } else {
        for (long long j = i; j < n; ++j) sgdm_elem(p[j], g[j], m[j], lr, wd, s, mom, nesterov);
    }
}

extern "C" int mt4_sgd_momentum_step_f32(float* p, const float* g, float* m, int64_t n, float lr, float weight_decay, float grad_scale,
                                         float momentum, int32_t nesterov, const mt4_guard_state* guard_state, void* stream) {
    mt4_clear_error();
    if (!p || !g || !m || n <= 0 || !(momentum >= 0.f && momentum < 1.f) || (nesterov && momentum == 0.f)) return MT4_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m) & 15) || ((uintptr_t)guard_state & 7)) return MT4_EINVAL;
    const long long threads = (n + 3) / 4;
    if ((threads + 255) / 256 > 0x7fffffffLL) return MT4_EINVAL;
    hipLaunchKernelGGL(sgd_momentum_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, (long long)n, lr,
                       weight_decay, grad_scale, momentum, nesterov ? 1 : 0, guard_state);
    return mt4_check_launch();
}

// torch.optim.AdamW (amsgrad off).  Per thread (K = the scalars every element shares):
//   s    = grad_scale * coef                     float
//   b1, b2 = (float)beta1, (float)beta2          float  (the betas arrive as doubles)
//   c1   = (float)(1.0 - beta1), c2 = (float)(1.0 - beta2)        the subtraction in double, one rounding to float
//   lw   = lr * wd                               float
//   step = (float)((double)lr / (1.0 - beta1_pow))                double subtraction and division, one rounding to float
//   r2   = (float)sqrt(1.0 - beta2_pow)                           double subtraction and square root, one rounding to float
// Per element, all float:
//   q = p - lw * p;   h = g * s;   m' = b1 * m + c1 * h;   v' = b2 * v + c2 * (h * h);   den = sqrt(v') / r2 + eps;   p' = q - step * (m' / den)
struct adamw_k {
    float s, b1, b2, c1, c2, lw, step, r2, eps;
};

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, const adamw_k& K) {
#pragma clang fp contract(off)
    const float lp = K.lw * p;
    const float q = p - lp;
    const float h = g * K.s;
    const float m1 = K.b1 * m;
    const float m2 = K.c1 * h;
    const float mn = m1 + m2;
    const float hh = h * h;
    const float v1 = K.b2 * v;
    const float v2 = K.c2 * hh;
    const float vn = v1 + v2;
    const float sq = sqrtf(vn);                 // correctly rounded (llvm.sqrt.f32 under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt);
    const float sr = sq / K.r2;                 // HIP's __fsqrt_rn is the native 1-ulp square root, so it is NOT used here; `/` is the IEEE quotient
    const float den = sr + K.eps;
    const float qu = mn / den;
    const float up = K.step * qu;
    p = q - up;
    m = mn;
    v = vn;
}

__global__ void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long long n, float lr,
                             float wd, float grad_scale, double beta1, double beta2, float eps, const mt4_optim_state* __restrict__ os,
                             const mt4_guard_state* __restrict__ guard) {
#pragma clang fp contract(off)
    if (guard && guard->skip) return;
    adamw_k K;
    K.s = guard ? grad_scale * guard->coef : grad_scale;
    K.b1 = (float)beta1;
    K.b2 = (float)beta2;
    K.c1 = (float)(1.0 - beta1);
    K.c2 = (float)(1.0 - beta2);
    K.lw = lr * wd;
    const double bc1 = 1.0 - os->beta1_pow, bc2 = 1.0 - os->beta2_pow;
    K.step = (float)((double)lr / bc1);
    K.r2 = (float)sqrt(bc2);
    K.eps = eps;
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i + 3 < n) {
        float4 pv = *(float4*)(p + i), mv = *(float4*)(m + i), vv = *(float4*)(v + i);
        const float4 gv = *(const float4*)(g + i);
        adamw_elem(pv.x, gv.x, mv.x, vv.x, K); adamw_elem(pv.y, gv.y, mv.y, vv.y, K);
        adamw_elem(pv.z, gv.z, mv.z, vv.z, K); adamw_elem(pv.w, gv.w, mv.w, vv.w, K);
        *(float4*)(p + i) = pv;
        *(float4*)(m + i) = mv;
        *(float4*)(v + i) = vv;
    } else {
        for (long long j = i; j < n; ++j) adamw_elem(p[j], g[j], m[j], v[j], K);
    }
}

extern "C" int mt4_adamw_step_f32(float* p, const float* g, float* m, float* v, int64_t n, float lr, float weight_decay, float grad_scale,
                                  double beta1, double beta2, float eps, const mt4_optim_state* optim_state, const mt4_guard_state* guard_state,
                                  void* stream) {
    mt4_clear_error();
    if (!p || !g || !m || !v || !optim_state || n <= 0 || !(beta1 >= 0. && beta1 < 1.) || !(beta2 >= 0. && beta2 < 1.) || !(eps > 0.f))
        return MT4_EINVAL;
    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) || (((uintptr_t)optim_state | (uintptr_t)guard_state) & 7)) return MT4_EINVAL;
    const long long threads = (n + 3) / 4;
    if ((threads + 255) / 256 > 0x7fffffffLL) return MT4_EINVAL;
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long long)n, lr,
                       weight_decay, grad_scale, beta1, beta2, eps, optim_state, guard_state);
    return mt4_check_launch();
}

// ------------------------------------------------------------------------------------------------ weight average (--ema_decay)
// E <- decay E + (1 - decay) P behind the parameter update, the decay of the step kept in a device record for the reason mt4_optim_state is: under
// --skip_nonfinite the host never learns whether a step counted.  `ops.ema_advance_host` / `ops.ema_step_host` restate both and give the same bits.

// one thread: unless the guard says skip, t += 1 and the step's decay d = warmup ? min(decay, (1 + t) / (10 + t)) : decay in IEEE double (the
// num_updates form of TensorFlow's ExponentialMovingAverage); decay = (float)d, comp = (float)(1.0 - d), each rounded once
__global__ void ema_advance_kernel(mt4_ema_state* __restrict__ es, double decay, int warmup, const mt4_guard_state* __restrict__ guard) {
    if (guard && guard->skip) return;
    const long long t = es->t + 1;
    double d = decay;
    if (warmup) {
        const double w = (1.0 + (double)t) / (10.0 + (double)t);
        if (w < d) d = w;
    }
    es->t = t;
    es->decay = (float)d;
    es->comp = (float)(1.0 - d);
}

extern "C" int mt4_ema_advance(mt4_ema_state* ema_state, double decay, int32_t warmup, const mt4_guard_state* guard_state, void* stream) {
    mt4_clear_error();
    if (!ema_state || !(decay >= 0. && decay < 1.)) return MT4_EINVAL;
    if (((uintptr_t)ema_state | (uintptr_t)guard_state) & 7) return MT4_EALIGN;
    hipLaunchKernelGGL(ema_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, ema_state, decay, warmup ? 1 : 0, guard_state);
    return mt4_check_launch();
}

#define EMA_THREADS 256
#define EMA_MAX_BLOCKS 2048LL     // 8 workgroups per CU: a longer buffer is walked with the grid's stride

// two multiplies and one add, each ONE round-to-nearest operation in this order.  HIP's __fmul_rn / __fadd_rn are the plain operators, which hipcc's
// default -ffp-contract=fast fuses into an FMA: the pragma (here and in the kernel body, as in sgdm_elem) is what keeps the three roundings
__device__ __forceinline__ float ema_elem(float e, float p, float d, float c) {
#pragma clang fp contract(off)
    const float de = d * e;
    const float cp = c * p;
    return de + cp;
}

// a pure stream of 12 bytes per element (e read and written, p read): 16-byte accesses, the n % 4 tail element by element in the thread whose
// float4 it would be
__global__ __launch_bounds__(EMA_THREADS) void ema_step_kernel(float* __restrict__ e, const float* __restrict__ p, long long n,
                                                               const mt4_ema_state* __restrict__ es, const mt4_guard_state* __restrict__ guard) {
#pragma clang fp contract(off)
    if (guard && guard->skip) return;
    const float d = es->decay, c = es->comp;
    const long long stride = (long long)gridDim.x * EMA_THREADS * 4;
    for (long long i = ((long long)blockIdx.x * EMA_THREADS + threadIdx.x) * 4; i < n; i += stride) {
        if (i + 3 < n) {
            float4 ev = *(float4*)(e + i);
            const float4 pv = *(const float4*)(p + i);
            ev.x = ema_elem(ev.x, pv.x, d, c); ev.y = ema_elem(ev.y, pv.y, d, c);
            ev.z = ema_elem(ev.z, pv.z, d, c); ev.w = ema_elem(ev.w, pv.w, d, c);
            *(float4*)(e + i) = ev;
        } else {
            for (long long j = i; j < n; ++j) e[j] = ema_elem(e[j], p[j], d, c);
        }
    }
}

extern "C" int mt4_ema_step_f32(float* e, const float* p, int64_t n, const mt4_ema_state* ema_state, const mt4_guard_state* guard_state,
                                void* stream) {
    mt4_clear_error();
    if (!e || !p || !ema_state || n <= 0) return MT4_EINVAL;
    if ((((uintptr_t)e | (uintptr_t)p) & 15) || (((uintptr_t)ema_state | (uintptr_t)guard_state) & 7)) return MT4_EALIGN;
    const long long threads = (n + 3) / 4;
    const long long blocks = min((threads + EMA_THREADS - 1) / EMA_THREADS, EMA_MAX_BLOCKS);
    hipLaunchKernelGGL(ema_step_kernel, dim3((unsigned)blocks), dim3(EMA_THREADS), 0, (hipStream_t)stream, e, p, (long long)n, ema_state,
                       guard_state);
    return mt4_check_launch();
}
