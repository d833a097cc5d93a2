// The streaming step of the causal temporal head on gfx950 (MI355X): a handful of NEW frames through one causal Conv1d against the layer's own
// history (`DilatedResidualCausalLayer`, Temporal_tenco/network.py:165-183: front padding 2 d, taps at t - 2d, t - d, t), fp32.
//
// Every layer keeps its input in a ring of L rows (L a power of two >= (taps - 1) d + 32): frame f lives in row f & (L - 1).  A launch computes the
// n <= 32 frames f = t0 + i, t0 read from a device counter; tap k of frame f is frame f - (taps - 1 - k) d of the input ring, or zeros when that
// frame is negative: the front padding is the counter, not a zero-filled buffer, so a reset is one store to the counter and no gather pass ever
// builds a contiguous window.
//
// The GEMM is skinny (<= 32 rows, K = taps Cin, Cout columns) and bound by the weight read.  Geometry of `tcn_conv_kernel` (tcn_kernels.hip): one
// workgroup per 16 output channels, K split over the 8 waves by 128-byte step (step s belongs to wave s & 7, a wave walks its steps upwards, six in flight), the 8
// partial tiles meet in LDS and are added in the order wave 0..7.  Each lane's operands come straight from global memory into registers (a weight
// element is used by one lane; the <= 32 x 128 bytes of frames per step are L2 hits shared by all workgroups), so there is no barrier in the K loop.
// An output element's sum therefore has ONE order, fixed by (taps, Cin) alone: not by n, the row's place in the chunk, t0 or the ring position --
// any two chunkings of a video give the same bits.
//
// The row-table form: one launch for one chunk of EACH of several videos (`tenco_stream.StreamBank`).  Row r of the launch is frame
// counters[row_slot[r]] + row_idx[r] of the stream in slot row_slot[r], whose rings are slice row_slot[r] of [n_slots][L][C] operands; blockIdx.y
// picks a block of 32 rows (two 16-row tiles, as a solo chunk) and the number of valid rows is a device word, so one captured launch serves any mix
// of per-stream counts.  Both forms are instantiations of ONE kernel body, `tcn_stream_conv_kernel<TAPS, K>`: they differ in where a block's rows
// come from and where they go, never in the K split, the step order inside a wave or the fold order, and an MFMA column is one row's sum -- a
// row's bits are those of its video's solo launch, whatever shares its launch, because there is no second K loop to drift from the first.
// Registers (gfx950): solo 174 VGPRs at three taps and 164 at one, table form 172 and 163; no scratch, 16 KB of LDS.
#include "mt4_common.h"

namespace {

constexpr int kStreamMaxChunk = 32, kStreamBN = 16, kStreamWaves = 8, kStreamMaxSlots = 64;

struct StreamK {
    static constexpr bool kTable = false;
    const float* x;        // input ring [Lin][Cin] (Lin == 0: plain [n][Cin])
    const float* w;        // [Cout][taps * Cin]
    const float* bias;     // [Cout] or NULL
    const float* res;      // residual ring [Lres][Cout] (Lres == 0: plain) or NULL
    float* y;              // output ring [Lout][Cout] (Lout == 0: plain)
    const long long* t0;   // frames pushed before this chunk
    int Lin, Lres, Lout;
    int Cin, Cout, d, n, relu;
    int SPT;               // 128-byte K-steps per tap
};

struct StreamRowsK {
    static constexpr bool kTable = true;
    const float* x;            // input rings [n_slots][Lin][Cin] (Lin == 0: plain [max_rows][Cin], row r)
    const float* w;            // [Cout][taps * Cin]
    const float* bias;         // [Cout] or NULL
    const float* res;          // residual rings [n_slots][Lres][Cout] (Lres == 0: plain) or NULL
    float* y;                  // output rings [n_slots][Lout][Cout] (Lout == 0: plain)
    const int* row_slot;       // [max_rows] the stream of row r
    const int* row_idx;        // [max_rows] which of that stream's new frames row r is, 0..31
    const int* n_rows;         // valid rows of this launch (<= max_rows)
    const long long* counters; // [n_slots] frames pushed before this chunk, per stream
    int Lin, Lres, Lout;
    int Cin, Cout, d, relu;
    int n_slots, max_rows;
    int SPT;                   // 128-byte K-steps per tap
};

template <int TAPS, typename K>
__global__ __launch_bounds__(kStreamWaves * 64) void tcn_stream_conv_kernel(const K a) {
    __shared__ f32x4 red[kStreamWaves * 2 * 64];
    // ---- (1) the block's first row of the launch and its valid rows
    int rb0 = 0, nb;
    if constexpr (K::kTable) {
        rb0 = blockIdx.y * kStreamMaxChunk;
        const int nr = min(*a.n_rows, a.max_rows);
        if (rb0 >= nr) return;                       // a block behind the valid rows: the whole workgroup, before any load or barrier
        nb = min(nr - rb0, kStreamMaxChunk);         // valid rows of this block, >= 1
    } else {
        nb = a.n;
    }
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    const int n0 = blockIdx.x * kStreamBN;
    long long t0 = 0;
    if constexpr (!K::kTable) t0 = *a.t0;
    const bool two = nb > 16;                        // a second 16-row tile (block-uniform)

    // ---- (2) a lane's two rows (tile mt: block row i = mt * 16 + r16): the frame, the buffer its ring rows count from and whether the row counts.
    // Lanes beyond the valid rows take the block's last valid row again (one more hit, no new line).  The table form reads its tables once, here,
    // ahead of the K loop: a slot or index outside its range is clamped for the loads and the row is not valid; a plain buffer's row r is put
    // into the base.  The solo form's row is arithmetic on t0 and n, which `load` spells out where it is consumed (the `K::kTable ? :` there):
    // passing it through these arrays computes the same thing, but the compiler then repeats the row's address arithmetic in every step
    long long tfr[2];
    const float* tx[2];
    bool tvalid[2];
    if constexpr (K::kTable) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int i = mt * 16 + r16, r = rb0 + min(i, nb - 1);
            const int slot = a.row_slot[r], idx = a.row_idx[r];
            const int sc = min(max(slot, 0), a.n_slots - 1), jc = min(max(idx, 0), kStreamMaxChunk - 1);
            tvalid[mt] = i < nb && slot == sc && idx == jc;
            tfr[mt] = a.counters[sc] + jc;
            tx[mt] = a.Lin ? a.x + (long long)sc * a.Lin * a.Cin : a.x + (long long)r * a.Cin;
        }
    }

    // this lane's B fragments: tap k of frame f is frame f - (TAPS - 1 - k) d of the ring, zeros when that frame is negative or the row does not count
    const int wn = min(n0 + r16, a.Cout - 1);        // rows >= Cout feed accumulator rows that are never stored
    const float* const wrow = a.w + (long long)wn * (TAPS * a.Cin) + q * 4;
    const int SPT = a.SPT, NS = TAPS * SPT;
    struct Frag { float4 w[2], x[2][2]; bool ok[2]; };
    // step s = tap * SPT + cs covers K elements [32 s, 32 s + 32) of the packed row
    auto load = [&](int s, Frag& f) {
        const int tap = TAPS == 1 ? 0 : (s >= SPT) + (s >= 2 * SPT);
        const int cs = s - tap * SPT;
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) f.w[kk] = *(const float4*)(wrow + s * 32 + kk * 16);
        // the loads are unconditional (a row that is always inside the buffer: any frame's ring row, a valid row of a plain buffer) and the
        // zeros are selected where the values are consumed (`compute`): a load under a per-lane condition becomes a branch and a full wait, and a
        // select behind the load waits for it there -- either way the ring of fragment sets is lost
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (mt == 1 && !two) break;
            const int i = mt * 16 + r16, ic = min(i, nb - 1);
            const long long fr = (K::kTable ? tfr[mt] : t0 + ic) - (long long)(TAPS - 1 - tap) * a.d;
            const long long row = a.Lin ? (fr & (long long)(a.Lin - 1)) : (long long)(K::kTable ? 0 : ic);
            f.ok[mt] = (K::kTable ? tvalid[mt] : i < nb) && fr >= 0;
            const float* xp = (K::kTable ? tx[mt] : a.x) + row * a.Cin + cs * 32 + q * 4;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) f.x[kk][mt] = *(const float4*)(xp + kk * 16);
        }
    };
    f32x4 acc[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
    auto compute = [&](const Frag& f) {
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if (mt == 1 && !two) break;
                const float4 v = f.x[kk][mt];
                const bool ok = f.ok[mt];
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.w[kk].x, ok ? v.x : 0.f, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.w[kk].y, ok ? v.y : 0.f, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.w[kk].z, ok ? v.z : 0.f, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(f.w[kk].w, ok ? v.w : 0.f, acc[mt], 0, 0, 0);
            }
        }
    };
    // wave w takes steps w, w + 8, ... in rising order through a ring of kDepth fragment sets: the loads of kDepth steps are in flight at once (at
    // K = 3 x 512 a wave has 6 steps: one round trip to memory for the whole K loop)
    constexpr int NW = kStreamWaves, kDepth = 6;
    Frag fs[kDepth];
    int s = wave;
#pragma unroll
    for (int j = 0; j < kDepth; ++j)
        if (s + j * NW < NS) load(s + j * NW, fs[j]);
    while (s < NS) {
#pragma unroll
        for (int j = 0; j < kDepth; ++j) {
            if (s + j * NW >= NS) break;
            compute(fs[j]);
            if (s + (j + kDepth) * NW < NS) load(s + (j + kDepth) * NW, fs[j]);
        }
        s += kDepth * NW;
    }

    // ---- partial tiles -> LDS, fixed-order sum and fused epilogue by waves 0 / 1 (row tile mt = wave)
    red[(wave * 2 + 0) * 64 + lane] = acc[0];
    red[(wave * 2 + 1) * 64 + lane] = acc[1];
    __syncthreads();
    if (wave >= 2) return;
    const int i = wave * 16 + r16;                   // row of the block
    const int en = n0 + q * 4;                       // Cout % 4 == 0: en < Cout implies en + 3 < Cout
    if (i >= nb || en >= a.Cout) return;
    // ---- (3) the row's frame, the first row of its stream's ring slice (in units of the ring) and its row in a plain buffer
    const int r = rb0 + i;
    long long f, slice = 0;
    if constexpr (K::kTable) {
        const int slot = a.row_slot[r], idx = a.row_idx[r];
        if (slot < 0 || slot >= a.n_slots || idx < 0 || idx >= kStreamMaxChunk) return;
        f = a.counters[slot] + idx;
        slice = slot;
    } else {
        f = t0 + i;
    }
    auto ring_row = [&](int L) { return L ? slice * L + (f & (long long)(L - 1)) : (long long)r; };
    f32x4 sum = red[wave * 64 + lane];
#pragma unroll
    for (int v = 1; v < kStreamWaves; ++v) sum += red[(v * 2 + wave) * 64 + lane];
    if (a.bias) {
        const float4 b = *(const float4*)(a.bias + en);
        sum += (f32x4){b.x, b.y, b.z, b.w};
    }
    if (a.res) {
        const float4 rv = *(const float4*)(a.res + ring_row(a.Lres) * a.Cout + en);
        sum += (f32x4){rv.x, rv.y, rv.z, rv.w};
    }
    if (a.relu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) sum[e] = fmaxf(sum[e], 0.f);
    }
    *(float4*)(a.y + ring_row(a.Lout) * a.Cout + en) = make_float4(sum[0], sum[1], sum[2], sum[3]);
}

__global__ void tcn_stream_advance_kernel(long long* t0, int n) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *t0 += n;
}

// counters[push_slot[a]] += push_count[a], a < *n_push: one thread per entry (the table names a slot once)
__global__ void tcn_stream_advance_rows_kernel(long long* counters, int n_slots, const int* push_slot, const int* push_count, const int* n_push) {
    const int a = threadIdx.x;
    if (blockIdx.x != 0 || a >= min(*n_push, n_slots)) return;
    const int slot = push_slot[a], c = push_count[a];
    if (slot < 0 || slot >= n_slots || c < 0 || c > kStreamMaxChunk) return;
    counters[slot] += c;
}

bool ring_ok(int L) { return L == 0 || (L > 0 && (L & (L - 1)) == 0); }

// what both conv entry points ask of their common arguments; chunk: the most frames one stream brings to the launch
int stream_conv_args(const float* x, int Lin, const float* residual, int Lres, const float* y, int Lout, const float* w, const float* bias, int Cin,
                     int Cout, int taps, int dilation, int relu, int chunk) {
    if (!x || !y || !w) return MT4_EINVAL;
    if (Cin <= 0 || Cout <= 0 || dilation <= 0 || (taps != 1 && taps != 3) || relu < 0 || relu > 1) return MT4_EINVAL;
    if (!ring_ok(Lin) || !ring_ok(Lres) || !ring_ok(Lout)) return MT4_EINVAL;
    if (taps == 3 && Lin == 0) return MT4_EINVAL;                                       // a history needs a ring
    if (Lin && Lin < (long long)(taps - 1) * dilation + chunk) return MT4_EINVAL;        // frames t0 - (taps - 1) d .. t0 + chunk - 1 must all be in the ring
    if ((Lres && Lres < chunk) || (Lout && Lout < chunk)) return MT4_EINVAL;
    if ((Cin * 4) % 128 != 0 || Cout % 4 != 0) return MT4_EUNSUPPORTED;
    if ((long long)taps * Cin * Cout > 0x3fffffffLL) return MT4_EUNSUPPORTED;
    if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)y | (uintptr_t)residual | (uintptr_t)bias) & 15) return MT4_EALIGN;
    return MT4_OK;
}

}  // namespace

extern "C" int mt4_tcn_stream_conv_f32(const float* x, int32_t Lin, const float* residual, int32_t Lres, float* y, int32_t Lout, const float* w,
                                       const float* bias, int32_t Cin, int32_t Cout, int32_t taps, int32_t dilation, int32_t relu, int32_t n,
                                       const int64_t* t0, void* stream) {
    mt4_clear_error();
    if (!t0 || n < 1 || n > kStreamMaxChunk) return MT4_EINVAL;
    if (const int rc = stream_conv_args(x, Lin, residual, Lres, y, Lout, w, bias, Cin, Cout, taps, dilation, relu, n)) return rc;
    if ((uintptr_t)t0 & 7) return MT4_EALIGN;
    StreamK k{x, w, bias, residual, y, (const long long*)t0, Lin, residual ? Lres : 0, Lout, Cin, Cout, taps == 1 ? 1 : dilation, n, relu, Cin * 4 / 128};
    const dim3 grid(cdiv(Cout, kStreamBN)), block(kStreamWaves * 64);
    if (taps == 3) return mt4_launch<tcn_stream_conv_kernel<3, StreamK>>(grid, block, 0, (hipStream_t)stream, k);
    return mt4_launch<tcn_stream_conv_kernel<1, StreamK>>(grid, block, 0, (hipStream_t)stream, k);
}

extern "C" int mt4_tcn_stream_conv_rows_f32(const float* x, int32_t Lin, const float* residual, int32_t Lres, float* y, int32_t Lout, const float* w,
                                            const float* bias, int32_t Cin, int32_t Cout, int32_t taps, int32_t dilation, int32_t relu,
                                            int32_t n_slots, int32_t max_rows, const int32_t* row_slot, const int32_t* row_idx,
                                            const int32_t* n_rows, const int64_t* counters, void* stream) {
    mt4_clear_error();
    if (!row_slot || !row_idx || !n_rows || !counters) return MT4_EINVAL;
    if (n_slots < 1 || n_slots > kStreamMaxSlots || max_rows < 1 || max_rows > kStreamMaxChunk * n_slots) return MT4_EINVAL;
    // a stream may bring a full chunk
    if (const int rc = stream_conv_args(x, Lin, residual, Lres, y, Lout, w, bias, Cin, Cout, taps, dilation, relu, kStreamMaxChunk)) return rc;
    if (((uintptr_t)counters & 7) || (((uintptr_t)row_slot | (uintptr_t)row_idx | (uintptr_t)n_rows) & 3)) return MT4_EALIGN;
    StreamRowsK k{x, w, bias, residual, y, (const int*)row_slot, (const int*)row_idx, (const int*)n_rows, (const long long*)counters,
                  Lin, residual ? Lres : 0, Lout, Cin, Cout, taps == 1 ? 1 : dilation, relu, n_slots, max_rows, Cin * 4 / 128};
    const dim3 grid(cdiv(Cout, kStreamBN), cdiv(max_rows, kStreamMaxChunk)), block(kStreamWaves * 64);
    if (taps == 3) return mt4_launch<tcn_stream_conv_kernel<3, StreamRowsK>>(grid, block, 0, (hipStream_t)stream, k);
    return mt4_launch<tcn_stream_conv_kernel<1, StreamRowsK>>(grid, block, 0, (hipStream_t)stream, k);
}

extern "C" int mt4_tcn_stream_advance_rows(int64_t* counters, int32_t n_slots, const int32_t* push_slot, const int32_t* push_count,
                                           const int32_t* n_push, void* stream) {
    mt4_clear_error();
    if (!counters || !push_slot || !push_count || !n_push || n_slots < 1 || n_slots > kStreamMaxSlots) return MT4_EINVAL;
    if (((uintptr_t)counters & 7) || (((uintptr_t)push_slot | (uintptr_t)push_count | (uintptr_t)n_push) & 3)) return MT4_EALIGN;
    hipLaunchKernelGGL(tcn_stream_advance_rows_kernel, dim3(1), dim3(kStreamMaxSlots), 0, (hipStream_t)stream, (long long*)counters, (int)n_slots,
                       (const int*)push_slot, (const int*)push_count, (const int*)n_push);
    return mt4_check_launch();
}

extern "C" int mt4_tcn_stream_advance(int64_t* t0, int32_t n, void* stream) {
    mt4_clear_error();
    if (!t0 || ((uintptr_t)t0 & 7) || n < 0 || n > kStreamMaxChunk) return MT4_EINVAL;
    hipLaunchKernelGGL(tcn_stream_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)t0, (int)n);
    return mt4_check_launch();
}
