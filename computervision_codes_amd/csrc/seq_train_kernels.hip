// Backward-pass pieces of the transformer-shaped temporal teacher (MS-TCT, `Temporal_mstct/MSTCT/Temporal_Encoder.py`, trained by
// `Temporal_mstct/run.py:147-235` through torch autograd): what autograd derives for nn.LayerNorm, the softmax attention of
// Global_Relational_Block (:76-88), nn.GELU and the depthwise Conv1d of Local_Relational_Block (:34-43).  fp32 throughout (the parity
// mode of the trainers); GEMM-shaped work runs on v_mfma_f32_16x16x4_f32 (exact fp32 FMA chain).
#include "mt4_common.h"

namespace {

// ------------------------------------------------------------------------------------------------ strided batched GEMM
// C[b1][b0] (M x N) = alpha * A[b1][b0] (M x K) . B[b1][b0] (K x N) (+ C when beta != 0); every operand is addressed by element strides,
// so transposes and head slices of packed projection buffers ([B*T][heads*hd]) need no copies.  64 x 64 tile per workgroup of four
// waves (2 x 2, wave tile 32 x 32 = 2 x 2 MFMA tiles), K-steps of 16 staged through LDS k-major (As[k][m], Bs[k][n]): the fragment of
// lane (r16, q) is one word of row k0 + q, so the 16 lanes of a quad read 16 consecutive words.
struct BgemmK {
    const float* A; const float* B; float* C;
    int M, N, K, nb0;
    long long a_b0, a_b1, a_m, a_k;
    long long b_b0, b_b1, b_k, b_n;
    long long c_b0, c_b1, c_m, c_n;
    float alpha; int beta;
};

__global__ __launch_bounds__(256) void bgemm_f32_kernel(const BgemmK p) {
    constexpr int BT = 64, KS = 16, LD = BT + 16;   // +16 words: the two quads of a 32-lane ds_read_b32 group land on disjoint banks
    __shared__ float As[2][KS][LD];
    __shared__ float Bs[2][KS][LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r16 = lane & 15, q = lane >> 4;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int b = blockIdx.z;
    const int b1 = b / p.nb0, b0 = b - b1 * p.nb0;
    const float* A = p.A + b0 * p.a_b0 + b1 * p.a_b1;
    const float* B = p.B + b0 * p.b_b0 + b1 * p.b_b1;
    float* C = p.C + b0 * p.c_b0 + b1 * p.c_b1;
    const int m0 = blockIdx.y * BT, n0 = blockIdx.x * BT;
    // staging map: 1024 elements per operand and K-step, 4 per thread.  k-fast when the operand is contiguous along k (16 lanes read
    // one 64-byte run), else m-fast / n-fast (64 lanes read one 256-byte run when that stride is 1)
    const bool a_kfast = p.a_k == 1, b_kfast = p.b_k == 1;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float ra[4], rb[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int ka = a_kfast ? (e & 15) : (e >> 6), ma = a_kfast ? (e >> 4) : (e & 63);
            const int kb = b_kfast ? (e & 15) : (e >> 6), nb = b_kfast ? (e >> 4) : (e & 63);
            ra[i] = (m0 + ma < p.M && k0 + ka < p.K) ? A[(long long)(m0 + ma) * p.a_m + (long long)(k0 + ka) * p.a_k] : 0.f;
            rb[i] = (n0 + nb < p.N && k0 + kb < p.K) ? B[(long long)(k0 + kb) * p.b_k + (long long)(n0 + nb) * p.b_n] : 0.f;
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = tid + 256 * i;
            const int ka = a_kfast ? (e & 15) : (e >> 6), ma = a_kfast ? (e >> 4) : (e & 63);
            const int kb = b_kfast ? (e & 15) : (e >> 6), nb = b_kfast ? (e >> 4) : (e & 63);
            As[buf][ka][ma] = ra[i];
            Bs[buf][kb][nb] = rb[i];
        }
    };
    const int nk = (p.K + KS - 1) / KS;
    fetch(0);
    stash(0);
    __syncthreads();
    for (int s = 0; s < nk; ++s) {
        const int buf = s & 1;
        if (s + 1 < nk) fetch((s + 1) * KS);          // next K-step's global loads fly during the MFMAs
#pragma unroll
        for (int kk = 0; kk < KS; kk += 4) {
            float fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = As[buf][kk + q][wm + i * 16 + r16];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = Bs[buf][kk + q][wn + j * 16 + r16];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (s + 1 < nk) stash(buf ^ 1);
        __syncthreads();
    }
    // accumulator lane (r16, q) holds rows m = 4q + e, column n = r16 of its 16 x 16 tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + j * 16 + r16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int m = m0 + wm + i * 16 + q * 4 + e;
                if (m < p.M && n < p.N) {
                    float* c = C + (long long)m * p.c_m + (long long)n * p.c_n;
                    const float v = p.alpha * acc[i][j][e];
                    *c = p.beta ? *c + v : v;
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------ softmax rows, forward and backward
// P = softmax(scale * S) in place; one wave per row, cols <= 64 * 16
__global__ __launch_bounds__(256) void softmax_rows_kernel(float* __restrict__ S, long long rows, int cols, float scale) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    float* s = S + row * cols;
    float v[16];
    float mx = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < cols ? s[c] * scale : -3.0e38f;
        mx = fmaxf(mx, v[i]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        v[i] = (lane + 64 * i) < cols ? __expf(v[i] - mx) : 0.f;
        sum += v[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < cols) s[c] = v[i] * inv;
    }
}

// dS = scale * P .* (dP - rowsum(P .* dP)), written over dP
__global__ __launch_bounds__(256) void softmax_bwd_rows_kernel(const float* __restrict__ P, float* __restrict__ dP, long long rows, int cols,
                                                                float scale) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* p = P + row * cols;
    float* d = dP + row * cols;
    float pv[16], dv[16];
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        pv[i] = c < cols ? p[c] : 0.f;
        dv[i] = c < cols ? d[c] : 0.f;
        dot += pv[i] * dv[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = lane + 64 * i;
        if (c < cols) d[c] = scale * pv[i] * (dv[i] - dot);
    }
}

// ------------------------------------------------------------------------------------------------ LayerNorm backward
// y = (x - mean) * rstd * gamma + beta over the last dimension (nn.LayerNorm, eps inside the sqrt, biased variance).
//   g = dy * gamma;  dx = rstd * (g - mean(g) - xhat * mean(g * xhat));  dgamma += sum_rows dy * xhat;  dbeta += sum_rows dy
// One wave per row at a time (C <= 64 * NI; NI = 16 / 32 / 48 by width), statistics recomputed from x; a wave keeps its dgamma / dbeta partial sums in registers
// over all its rows and adds them to the (caller-zeroed or accumulating) gradient buffers once, with float atomics.
template <int NI>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ gamma,
                                                             float* __restrict__ dx, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                             long long M, int C, float eps, int add_dx) {
    const int lane = threadIdx.x & 63;
    const long long wave = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long nwaves = (long long)gridDim.x * 4;
    float gm[NI], pg[NI], pb[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = lane + 64 * i;
        gm[i] = c < C ? gamma[c] : 0.f;
        pg[i] = pb[i] = 0.f;
    }
    const float invC = 1.0f / (float)C;
    for (long long row = wave; row < M; row += nwaves) {
        const float* xr = x + row * C;
        const float* dr = dy + row * C;
        float xv[NI], dv[NI];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane + 64 * i;
            xv[i] = c < C ? xr[c] : 0.f;
            dv[i] = c < C ? dr[c] : 0.f;
            s += xv[i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float mean = s * invC;
        float var = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float d = (lane + 64 * i) < C ? xv[i] - mean : 0.f;
            var += d * d;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) var += __shfl_xor(var, o);
        const float rstd = rsqrtf(var * invC + eps);
        float sg = 0.f, sgx = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const float xh = (xv[i] - mean) * rstd;
            const float g = dv[i] * gm[i];
            xv[i] = xh;                 // keep xhat
            sg += g;
            sgx += g * xh;
            pg[i] += dv[i] * xh;
            pb[i] += dv[i];
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { sg += __shfl_xor(sg, o); sgx += __shfl_xor(sgx, o); }
        sg *= invC;
        sgx *= invC;
        float* dxr = dx + row * C;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = lane + 64 * i;
            if (c < C) {
                const float v = rstd * (dv[i] * gm[i] - sg - xv[i] * sgx);
                dxr[c] = add_dx ? dxr[c] + v : v;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = lane + 64 * i;
        if (c < C) {
            atomicAdd(dgamma + c, pg[i]);
            atomicAdd(dbeta + c, pb[i]);
        }
    }
}

// ------------------------------------------------------------------------------------------------ GELU backward (erf form)
// dx = dy * (Phi(x) + x phi(x)),  Phi by the Abramowitz-Stegun 7.1.26 erf (|err| < 1.5e-7; shares its exp with phi), phi(x) = exp(-x^2/2) / sqrt(2 pi)
__global__ void gelu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ dx, long long n) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 d4 = *(const float4*)(dy + i);
    const float4 x4 = *(const float4*)(x + i);
    const float dd[4] = {d4.x, d4.y, d4.z, d4.w}, xx[4] = {x4.x, x4.y, x4.z, x4.w};
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float v = xx[e];
        const float ax = fabsf(v) * 0.70710678118654752440f;
        const float t = __frcp_rn(fmaf(0.3275911f, ax, 1.0f));
        float pl = fmaf(1.061405429f, t, -1.453152027f);
        pl = fmaf(pl, t, 1.421413741f);
        pl = fmaf(pl, t, -0.284496736f);
        pl = fmaf(pl, t, 0.254829592f);
        const float ex = __expf(-ax * ax);                       // exp(-x^2/2)
        const float erfa = 1.0f - pl * t * ex;
        const float Phi = 0.5f * (1.0f + copysignf(erfa, v));
        o[e] = dd[e] * (Phi + v * 0.3989422804014327f * ex);
    }
    *(float4*)(dx + i) = make_float4(o[0], o[1], o[2], o[3]);
}

// nn.GELU forward on a saved pre-activation (the training step keeps both): the same gelu_erf as the fused epilogues
__global__ void gelu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 v = *(const float4*)(x + i);
    *(float4*)(y + i) = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
}

// ------------------------------------------------------------------------------------------------ depthwise Conv1d k = 3 backward
// y[t][c] = b[c] + sum_k w[c][k] x[t + k - 1][c] per sequence of T frames (zero padding).
//   dx[t][c] = w[c][0] dy[t+1][c] + w[c][1] dy[t][c] + w[c][2] dy[t-1][c]
//   dw[c][k] += sum_t dy[t][c] x[t + k - 1][c];   db[c] += sum_t dy[t][c]
// One thread per channel over a slab of rows of one sequence (coalesced across channels); partial sums -> float atomics.  The slab's sums run
// in float64: one large product at the head of a slab (a sequence's first frame) would otherwise make each of the 31 later fp32 additions round
// at its size -- measured 1.7 x sqrt(T) 2^-24 sum |dy x| on such rows; the kernel is bound by its loads and the four v_fma_f64 per row hide there.
__global__ void dwconv1d_k3_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ w,
                                       float* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db, int T, int C, int slab) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const int seq = blockIdx.z, t0 = blockIdx.y * slab;
    const int t1 = min(T, t0 + slab);
    const long long base = (long long)seq * T * C + c;
    const float w0 = w[c * 3 + 0], w1 = w[c * 3 + 1], w2 = w[c * 3 + 2];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, ab = 0.0;
    float dprev = t0 > 0 ? dy[base + (long long)(t0 - 1) * C] : 0.f;
    float dcur = dy[base + (long long)t0 * C];
    float xprev = t0 > 0 ? x[base + (long long)(t0 - 1) * C] : 0.f;
    float xcur = x[base + (long long)t0 * C];
    for (int t = t0; t < t1; ++t) {
        const float dnext = t + 1 < T ? dy[base + (long long)(t + 1) * C] : 0.f;
        const float xnext = t + 1 < T ? x[base + (long long)(t + 1) * C] : 0.f;
        dx[base + (long long)t * C] = w0 * dnext + w1 * dcur + w2 * dprev;
        const double dc = (double)dcur;
        a0 += dc * xprev;
        a1 += dc * xcur;
        a2 += dc * xnext;
        ab += dc;
        dprev = dcur; dcur = dnext;
        xprev = xcur; xcur = xnext;
    }
    atomicAdd(dw + c * 3 + 0, (float)a0);
    atomicAdd(dw + c * 3 + 1, (float)a1);
    atomicAdd(dw + c * 3 + 2, (float)a2);
    atomicAdd(db + c, (float)ab);
}

// y = a * x + b * y   (gradient fan-in, summed mixer weights)
__global__ void axpby_kernel(const float* __restrict__ x, float* __restrict__ y, long long n, float a, float b) {
    const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float4 xv = *(const float4*)(x + i);
    float4 yv = b != 0.f ? *(const float4*)(y + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    yv.x = a * xv.x + b * yv.x; yv.y = a * xv.y + b * yv.y; yv.z = a * xv.z + b * yv.z; yv.w = a * xv.w + b * yv.w;
    *(float4*)(y + i) = yv;
}

// nn.Dropout(p) mask from a counter generator: element i = splitmix64(base + i), base = splitmix64(seed * 0x100000001B3 + stream) -- the
// same function as computervision_codes_amd/synth.py:uniform01, so the host can reproduce a draw bit for bit.
// out[i] = u_i >= p ? 1 / (1 - p) : 0
__global__ void dropout_mask_kernel(float* __restrict__ out, long long n, unsigned long long base, float p, float keep_scale) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double u = (double)(splitmix64(base + (unsigned long long)i) >> 11) * (1.0 / 9007199254740992.0);
    out[i] = u >= (double)p ? keep_scale : 0.f;
}


// ------------------------------------------------------------------------------------------------ row gather / scatter by a per-image map
// Swin's roll + window_partition (swin_transformer.py:241-252) and PatchMerging's 2x2 gather (:320-324) as seen from the training step:
//   gather : y[m][g*C + c] = x[(m / l_out) * l_in + map[(m % l_out) * group + g]][c]
//   scatter: x[(m / l_out) * l_in + map[(m % l_out) * group + g]][c] = y[m][g*C + c]      (the maps are bijections: plain stores)
__global__ void gather_rows_kernel(const float* __restrict__ x, const int* __restrict__ map, float* __restrict__ y, long long m_out, int C, int group,
                                   int l_out, int l_in, int scatter) {
    const int c4 = C >> 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;      // one float4 of one (m, g)
    const long long total = m_out * group * c4;
    if (i >= total) return;
    const int c = (int)(i % c4) * 4;
    const long long mg = i / c4;
    const int g = (int)(mg % group);
    const long long m = mg / group;
    const long long img = m / l_out;
    const int lo = (int)(m - img * l_out);
    const long long src = img * l_in + map[lo * group + g];
    float* yp = y + (m * group + g) * C + c;
    float* xp = const_cast<float*>(x) + src * C + c;
    if (scatter) *(float4*)xp = *(const float4*)yp;
    else *(float4*)yp = *(const float4*)xp;
}

// attention scores of a Swin block: S[bw][h][i][j] += bias[h][i][j] (+ mask[bw % nW][i][j])   (swin_transformer.py:127-136)
__global__ void add_bias_mask_kernel(float* __restrict__ S, const float* __restrict__ bias, const int* __restrict__ index,
                                     const float* __restrict__ mask, long long total, int H, int NN, int nW) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ij = (int)(i % NN);
    const long long bh = i / NN;
    const int h = (int)(bh % H);
    const long long bw = bh / H;
    // index: `bias` is the relative-position table [(2ws-1)^2][H] read through relative_position_index (swin_transformer.py:127-130)
    float v = S[i] + (index ? bias[(long long)index[ij] * H + h] : bias[(long long)h * NN + ij]);
    if (mask) v += mask[(bw % nW) * NN + ij];
    S[i] = v;
}

// gradient of the relative-position bias table: dtable[idx[ij]][h] += sum_bw dS[bw][h][ij]   (the gather of swin_transformer.py:127-130
// transposed).  A workgroup owns one head and a run of `per` windows: every thread sums its (i, j) positions over the run in registers
// (coalesced reads, four windows in flight), folds them into an LDS copy of the head's table column (ds_add_f32; many (i, j) share a row) and
// the workgroup adds that column to the table once -- (2ws-1)^2 global atomics per workgroup instead of one per (i, j).
__global__ __launch_bounds__(256) void relpos_table_grad_kernel(const float* __restrict__ dS, const int* __restrict__ idx, float* __restrict__ dtable,
                                                                long long nbw, int H, int NN, int TS, int per) {
    extern __shared__ float tab[];
    const int h = blockIdx.x;
    const long long w0 = (long long)blockIdx.y * per;
    const long long w1 = w0 + per < nbw ? w0 + per : nbw;
    for (int t = threadIdx.x; t < TS; t += 256) tab[t] = 0.f;
    __syncthreads();
    const long long st = (long long)H * NN;
    for (int ij = threadIdx.x; ij < NN; ij += 256) {
        const float* p = dS + (w0 * H + h) * (long long)NN + ij;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        long long w = w0;
        for (; w + 4 <= w1; w += 4, p += 4 * st) {
            s0 += p[0];
            s1 += p[st];
            s2 += p[2 * st];
            s3 += p[3 * st];
        }
        for (; w < w1; ++w, p += st) s0 += p[0];
        atomicAdd(&tab[idx[ij]], (s0 + s1) + (s2 + s3));
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TS; t += 256) atomicAdd(dtable + (long long)t * H + h, tab[t]);
}

// y[m][:] = s[m / rows_per_scale] * x[m][:] (+ r[m][:])   -- DropPath (timm, per-sample keep mask / keep_prob) on a residual branch
__global__ void rowscale_add_kernel(const float* __restrict__ x, const float* __restrict__ s, const float* __restrict__ r, float* __restrict__ y,
                                    long long M, int C, int rows_per_scale) {
    const int c4 = C >> 2;
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * c4) return;
    const long long m = i / c4;
    const float sc = s[m / rows_per_scale];
    const float4 xv = *(const float4*)(x + i * 4);
    float4 o = make_float4(sc * xv.x, sc * xv.y, sc * xv.z, sc * xv.w);
    if (r) { const float4 rv = *(const float4*)(r + i * 4); o.x += rv.x; o.y += rv.y; o.z += rv.z; o.w += rv.w; }
    *(float4*)(y + i * 4) = o;
}

// GroupWiseLinear backward (Spatial_transformer/network.py:40-45: out[b][k] = sum_d W[k][d] hs[b][k][d] + bias[k]):
//   dhs[b][k][d] = dy[b][k] W[k][d];  dW[k][d] += sum_b dy[b][k] hs[b][k][d];  db[k] += sum_b dy[b][k]
__global__ void groupwise_linear_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ hs, const float* __restrict__ W,
                                            float* __restrict__ dhs, float* __restrict__ dW, float* __restrict__ db, int B, int K, int D) {
    const int k = blockIdx.x;
    for (int d = threadIdx.x; d < D; d += blockDim.x) {
        const float w = W[(long long)k * D + d];
        float acc = 0.f;
        for (int b = 0; b < B; ++b) {
            const float g = dy[(long long)b * K + k];
            acc += g * hs[((long long)b * K + k) * D + d];
            dhs[((long long)b * K + k) * D + d] = g * w;
        }
        dW[(long long)k * D + d] += acc;
    }
    if (threadIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += dy[(long long)b * K + k];
        db[k] += s;
    }
}

// out[l][:] (+)= sum_b x[b*L + l][:]   (gradient of a row-broadcast add: the query embedding added to every image's queries)
__global__ void sum_over_batch_kernel(const float* __restrict__ x, float* __restrict__ out, int B, long long LC, int accumulate) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= LC) return;
    float s = accumulate ? out[i] : 0.f;
    for (int b = 0; b < B; ++b) s += x[(long long)b * LC + i];
    out[i] = s;
}

}  // namespace

extern "C" int mt4_gather_rows_f32(const float* x, const int32_t* map, float* y, int64_t m_out, int32_t C, int32_t group, int32_t l_out, int32_t l_in,
                                   int32_t scatter, void* stream) {
    mt4_clear_error();
    if (!x || !map || !y || m_out <= 0 || C <= 0 || (C & 3) || group <= 0 || l_out <= 0 || l_in <= 0) return MT4_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y) & 15) return MT4_EALIGN;
    const long long total = m_out * group * (C >> 2);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, map, y, (long long)m_out, C, group,
                       l_out, l_in, scatter ? 1 : 0);
    return mt4_check_launch();
}

extern "C" int mt4_add_bias_mask_f32(float* S, const float* bias, const int32_t* index, const float* mask, int64_t n_windows, int32_t heads, int32_t N,
                                     int32_t nW, void* stream) {
    mt4_clear_error();
    if (!S || !bias || n_windows <= 0 || heads <= 0 || N <= 0 || (mask && nW <= 0)) return MT4_EINVAL;
    const long long total = n_windows * heads * (long long)N * N;
    hipLaunchKernelGGL(add_bias_mask_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, S, bias, index, mask, total, heads,
                       N * N, mask ? nW : 1);
    return mt4_check_launch();
}

extern "C" int mt4_relpos_table_grad_f32(const float* dS, const int32_t* index, float* dtable, int64_t n_windows, int32_t heads, int32_t N, void* stream) {
    mt4_clear_error();
    if (!dS || !index || !dtable || n_windows <= 0 || heads <= 0 || N <= 0 || heads > 65535) return MT4_EINVAL;
    const int NN = N * N;
    int ws = 1;
    while (ws * ws < N) ++ws;
    if (ws * ws != N) return MT4_EINVAL;
    const int TS = (2 * ws - 1) * (2 * ws - 1);
    // ~2 workgroups per CU over heads x window runs; a run of >= 4 windows keeps four loads in flight per thread
    long long per = (n_windows * heads + 511) / 512;
    if (per < 4) per = 4;
    if (per > n_windows) per = n_windows;
    const long long zs = (n_windows + per - 1) / per;
    if (zs > 65535) return MT4_EUNSUPPORTED;
    hipLaunchKernelGGL(relpos_table_grad_kernel, dim3(heads, (unsigned)zs), dim3(256), TS * sizeof(float), (hipStream_t)stream, dS, index, dtable,
                       (long long)n_windows, heads, NN, TS, (int)per);
    return mt4_check_launch();
}

extern "C" int mt4_rowscale_add_f32(const float* x, const float* scale, const float* r, float* y, int64_t M, int32_t C, int32_t rows_per_scale, void* stream) {
    mt4_clear_error();
    if (!x || !scale || !y || M <= 0 || C <= 0 || (C & 3) || rows_per_scale <= 0) return MT4_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)r) & 15) return MT4_EALIGN;
    const long long total = M * (C >> 2);
    hipLaunchKernelGGL(rowscale_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, scale, r, y, (long long)M, C,
                       rows_per_scale);
    return mt4_check_launch();
}

extern "C" int mt4_groupwise_linear_bwd_f32(const float* dy, const float* hs, const float* W, float* dhs, float* dW, float* db, int32_t B, int32_t K,
                                            int32_t D, void* stream) {
    mt4_clear_error();
    if (!dy || !hs || !W || !dhs || !dW || !db || B <= 0 || K <= 0 || D <= 0) return MT4_EINVAL;
    hipLaunchKernelGGL(groupwise_linear_bwd_kernel, dim3(K), dim3(256), 0, (hipStream_t)stream, dy, hs, W, dhs, dW, db, B, K, D);
    return mt4_check_launch();
}

extern "C" int mt4_sum_over_batch_f32(const float* x, float* out, int32_t B, int64_t LC, int32_t accumulate, void* stream) {
    mt4_clear_error();
    if (!x || !out || B <= 0 || LC <= 0) return MT4_EINVAL;
    hipLaunchKernelGGL(sum_over_batch_kernel, dim3((unsigned)((LC + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out, B, (long long)LC, accumulate ? 1 : 0);
    return mt4_check_launch();
}

extern "C" int mt4_dropout_mask_f32(float* out, int64_t n, int64_t seed, int64_t stream_id, float p, void* stream) {
    mt4_clear_error();
    if (!out || n <= 0 || p < 0.f || p >= 1.f) return MT4_EINVAL;
    const unsigned long long base = splitmix64((unsigned long long)seed * 0x100000001B3ULL + (unsigned long long)stream_id);
    hipLaunchKernelGGL(dropout_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, out, (long long)n, base, p,
                       1.0f / (1.0f - p));
    return mt4_check_launch();
}

extern "C" int mt4_bgemm_f32(const float* A, const float* B, float* C, int32_t M, int32_t N, int32_t K, int32_t nb0, int32_t nb1,
                             const int64_t a_strides[4], const int64_t b_strides[4], const int64_t c_strides[4], float alpha, int32_t accumulate,
                             void* stream) {
    mt4_clear_error();
    if (!A || !B || !C || M <= 0 || N <= 0 || K <= 0 || nb0 <= 0 || nb1 <= 0 || !a_strides || !b_strides || !c_strides) return MT4_EINVAL;
    if ((long long)nb0 * nb1 > 65535) return MT4_EUNSUPPORTED;
    BgemmK p{A, B, C, M, N, K, nb0, a_strides[0], a_strides[1], a_strides[2], a_strides[3], b_strides[0], b_strides[1], b_strides[2], b_strides[3],
             c_strides[0], c_strides[1], c_strides[2], c_strides[3], alpha, accumulate ? 1 : 0};
    hipLaunchKernelGGL(bgemm_f32_kernel, dim3(cdiv(N, 64), cdiv(M, 64), nb0 * nb1), dim3(256), 0, (hipStream_t)stream, p);
    return mt4_check_launch();
}

extern "C" int mt4_softmax_rows_f32(float* S, int64_t rows, int32_t cols, float scale, void* stream) {
    mt4_clear_error();
    if (!S || rows <= 0 || cols <= 0) return MT4_EINVAL;
    if (cols > 1024) return MT4_EUNSUPPORTED;
    hipLaunchKernelGGL(softmax_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, S, (long long)rows, cols, scale);
    return mt4_check_launch();
}

extern "C" int mt4_softmax_bwd_rows_f32(const float* P, float* dP, int64_t rows, int32_t cols, float scale, void* stream) {
    mt4_clear_error();
    if (!P || !dP || rows <= 0 || cols <= 0) return MT4_EINVAL;
    if (cols > 1024) return MT4_EUNSUPPORTED;
    hipLaunchKernelGGL(softmax_bwd_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, P, dP, (long long)rows, cols, scale);
    return mt4_check_launch();
}

extern "C" int mt4_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, float* dx, float* dgamma, float* dbeta, int64_t M,
                                     int32_t C, float eps, int32_t accumulate_dx, void* stream) {
    mt4_clear_error();
    if (!dy || !x || !gamma || !dx || !dgamma || !dbeta || M <= 0 || C <= 0) return MT4_EINVAL;
    if (C > 3072) return MT4_EUNSUPPORTED;
    long long blocks = (M + 31) / 32;                       // a wave takes ~8 rows: few atomics, enough waves
    if (blocks > 1024) blocks = 1024;
    if (blocks < 1) blocks = 1;
    auto kern = C <= 1024 ? layernorm_bwd_kernel<16> : C <= 2048 ? layernorm_bwd_kernel<32> : layernorm_bwd_kernel<48>;
    hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dy, x, gamma, dx, dgamma, dbeta, (long long)M, C, eps,
                       accumulate_dx ? 1 : 0);
    return mt4_check_launch();
}

extern "C" int mt4_gelu_bwd_f32(const float* dy, const float* x, float* dx, int64_t n, void* stream) {
    mt4_clear_error();
    if (!dy || !x || !dx || n <= 0 || (n & 3)) return MT4_EINVAL;
    if (((uintptr_t)dy | (uintptr_t)x | (uintptr_t)dx) & 15) return MT4_EALIGN;
    hipLaunchKernelGGL(gelu_bwd_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy, x, dx, (long long)n);
    return mt4_check_launch();
}

extern "C" int mt4_gelu_f32(const float* x, float* y, int64_t n, void* stream) {
    mt4_clear_error();
    if (!x || !y || n <= 0 || (n & 3)) return MT4_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y) & 15) return MT4_EALIGN;
    hipLaunchKernelGGL(gelu_fwd_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n);
    return mt4_check_launch();
}

extern "C" int mt4_dwconv1d_k3_bwd_f32(const float* dy, const float* x, const float* w, float* dx, float* dw, float* db, int32_t B, int32_t T,
                                       int32_t C, void* stream) {
    mt4_clear_error();
    if (!dy || !x || !w || !dx || !dw || !db || B <= 0 || T <= 0 || C <= 0) return MT4_EINVAL;
    if (B > 65535) return MT4_EUNSUPPORTED;
    const int slab = 32;
    hipLaunchKernelGGL(dwconv1d_k3_bwd_kernel, dim3(cdiv(C, 256), cdiv(T, slab), B), dim3(256), 0, (hipStream_t)stream, dy, x, w, dx, dw, db, T, C, slab);
    return mt4_check_launch();
}

extern "C" int mt4_axpby_f32(const float* x, float* y, int64_t n, float a, float b, void* stream) {
    mt4_clear_error();
    if (!x || !y || n <= 0 || (n & 3)) return MT4_EINVAL;
    if (((uintptr_t)x | (uintptr_t)y) & 15) return MT4_EALIGN;
    hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long long)n, a, b);
    return mt4_check_launch();
}
