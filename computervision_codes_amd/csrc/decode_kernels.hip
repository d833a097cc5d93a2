// Decoding logits into an answer (computervision_codes_amd/predict.py): per row the k largest of up to 256 columns with their column ids, and how
// many columns lie above a threshold.  No reference counterpart: its drivers rank scores against labels only (`Temporal_mstct/run.py:507-523`).
//
// Order: descending by value as floats compare, equal values (+0.0 and -0.0 are equal) lower column first -- the first k entries of
// `torch.sort(x, dim=1, descending=True, stable=True)`.  The comparison runs on (float value, column) pairs and never on the raw bit pattern,
// which would put +0.0 in front of -0.0; the values written are the input's bits.  NaN is outside the contract (every comparison with it is
// false: the result is some permutation or the empty slot's column id, never an access out of bounds -- column ids are written, not followed).
//
// One wave owns a row.  Lane l holds columns l, l + 64, l + 128, l + 192 (the row-major load is coalesced), 4 "alive" bits say which are still
// in the race.  A round: the lane's best alive (value, column) -- slots ascend with the column, a strict > keeps the lower one --, four DPP
// exchange steps and four lane reads of the pairs after which every lane holds the wave's winner (`tk_wave_best`: no LDS traffic), the owner
// lane retires the slot, lane j keeps the winner of round j.  After k rounds lanes 0..k-1 store ids and values side by side (two coalesced
// vector stores per row).  An empty slot is (-inf, TK_NONE): it loses against a real -inf by the column rule, and k <= cols leaves a real
// candidate in every round.
//
// Two layouts, neither walks global memory with the long stride:
//   rows   x[r * row_stride + c]: four rows per 256-thread workgroup, a wave reads its row directly (64 consecutive floats per load).
//   cols   x[c * col_stride + r] ([K, T]: the unit stride runs along the rows): a 1024-thread workgroup stages cols x 16 rows in LDS -- a wave-load
//          covers 4 columns x 16 consecutive rows (64-byte runs; the neighbouring workgroups read the rest of each 128-byte line out of L2), all of
//          a wave's up to 4 loads in flight before the first LDS write -- and each of the 16 waves then takes its row out of LDS and ranks it.
//          LDS pitch 17 words: a row read has lane l at word (l + 64 s) * 17 + r, bank (17 l + const) % 32 -- a bijection within each 32-lane
//          group of a 4-byte read: conflict-free; the staging write puts lanes 16 g .. 16 g + 15 on 16 consecutive words 17 g apart: 2-way on
//          one bank per 32-lane group (reasoned from the bank rule, not measured with counters).
//          Measured for [2000, 100], k = 5 (profiles/r13_predict.txt; row-major 4.9 us): cols x 64 rows per 1024-thread workgroup, four rows per
//          wave, 19.2 us -- 2000 rows are 32 such tiles, so 32 of the 256 compute units ranked 64 rows each (~80 wave-instructions per row and
//          round) while row-major spreads 8 rows per unit; 16-row tiles (125 workgroups) with two rows per wave 8.3 us; one row per wave 6.1 us.
#include "mt4_common.h"

namespace {

constexpr int TK_MAX_COLS = 256, TK_MAX_K = 32, TK_SLOTS = TK_MAX_COLS / 64;
constexpr int TK_NONE = 1 << 30;                       // the column id of an empty slot: above every real column
constexpr int TK_TILE_ROWS = 16, TK_TILE_PITCH = TK_TILE_ROWS + 1, TK_TILE_WAVES = 16, TK_ROWS_PER_WAVE = TK_TILE_ROWS / TK_TILE_WAVES;
constexpr int TK_COLS_PER_LOAD = 64 / TK_TILE_ROWS, TK_STAGE_LOADS = TK_MAX_COLS / (TK_TILE_WAVES * TK_COLS_PER_LOAD);

// (v, c) := the better of (v, c) and (ov, oc)
__device__ __forceinline__ void tk_better(float& v, int& c, float ov, int oc) {
    const bool take = ov > v || (ov == v && oc < c);
    v = take ? ov : v;
    c = take ? oc : c;
}

// one exchange step inside a row of 16 lanes by a DPP lane pattern (every source lane exists: no bound handling)
template <int CTRL>
__device__ __forceinline__ void tk_dpp_step(float& v, int& c) {
    const float ov = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, 0xF, 0xF, false));
    const int oc = __builtin_amdgcn_update_dpp(c, c, CTRL, 0xF, 0xF, false);
    tk_better(v, c, ov, oc);
}

// every lane := the wave's best pair, without the LDS pipe (a `__shfl_xor` butterfly is 12 ds_bpermute per round and row, and the [K, T]
// kernel ranks 64 rows on ONE compute unit): quad_perm [1,0,3,2] and [2,3,0,1] make quads uniform, row_half_mirror (lane i <- 7 - i: the other
// quad of its 8) and row_mirror (i <- 15 - i: the other 8 of its 16) make the four rows of 16 uniform, four v_readlane pairs combine the rows.
// All 64 lanes are active wherever this runs.  The order is total on the pairs present (k <= cols), so any exchange order gives the same winner.
__device__ __forceinline__ void tk_wave_best(float& v, int& c) {
    tk_dpp_step<0xB1>(v, c);
    tk_dpp_step<0x4E>(v, c);
    tk_dpp_step<0x141>(v, c);
    tk_dpp_step<0x140>(v, c);
    float rv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    int rc = __builtin_amdgcn_readlane(c, 0);
#pragma unroll
    for (int l = 16; l < 64; l += 16)
        tk_better(rv, rc, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)), __builtin_amdgcn_readlane(c, l));
    v = rv;
    c = rc;
}

// R rows at once: val[q][s] = column lane + 64 s of row q (anything where that column is >= cols).  Leaves in lane j < k the j-th largest
// (value, column) of every row in (out_v[q], out_c[q]) and in every lane the row's count of columns > above in n_above[q].
template <int R>
__device__ __forceinline__ void tk_select(const float (&val)[R][TK_SLOTS], int cols, int k, float above, float (&out_v)[R], int (&out_c)[R],
                                          int (&n_above)[R]) {
    const int lane = threadIdx.x & 63;
    unsigned alive[R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
        alive[q] = 0u;
        int n = 0;
#pragma unroll
        for (int s = 0; s < TK_SLOTS; ++s) {
            const bool in = lane + 64 * s < cols;
            alive[q] |= in ? 1u << s : 0u;
            n += (in && val[q][s] > above) ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
        n_above[q] = n;
        out_v[q] = 0.f;
        out_c[q] = TK_NONE;
    }
    for (int j = 0; j < k; ++j) {
        float bv[R];
        int bc[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            bv[q] = -__builtin_inff();
            bc[q] = TK_NONE;
#pragma unroll
            for (int s = 0; s < TK_SLOTS; ++s) {
                const bool take = (alive[q] >> s & 1u) && (bc[q] == TK_NONE || val[q][s] > bv[q]);
                bv[q] = take ? val[q][s] : bv[q];
                bc[q] = take ? lane + 64 * s : bc[q];
            }
        }
#pragma unroll
        for (int q = 0; q < R; ++q) {
            tk_wave_best(bv[q], bc[q]);
            if ((bc[q] & 63) == lane && bc[q] != TK_NONE) alive[q] &= ~(1u << ((bc[q] >> 6) & 3));
            if (lane == j) { out_v[q] = bv[q]; out_c[q] = bc[q]; }
        }
    }
}

__device__ __forceinline__ void tk_store(long long row, int k, float v, int c, int n, int* __restrict__ ids, float* __restrict__ vals,
                                         int* __restrict__ n_above) {
    const int lane = threadIdx.x & 63;
    if (lane < k) {
        ids[row * k + lane] = c;
        vals[row * k + lane] = v;
    }
    if (n_above && lane == 0) n_above[row] = n;
}

__global__ __launch_bounds__(256) void topk_rowmajor_kernel(const float* __restrict__ x, long long rows, int cols, long long row_stride, int k,
                                                            float above, int* __restrict__ ids, float* __restrict__ vals, int* __restrict__ n_above) {
    const int lane = threadIdx.x & 63;
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                                       // (wave-uniform; the kernel has no barrier)
    const float* xr = x + row * row_stride;
    float val[1][TK_SLOTS];
#pragma unroll
    for (int s = 0; s < TK_SLOTS; ++s) val[0][s] = lane + 64 * s < cols ? xr[lane + 64 * s] : 0.f;
    float v[1];
    int c[1], n[1];
    tk_select<1>(val, cols, k, above, v, c, n);
    tk_store(row, k, v[0], c[0], n[0], ids, vals, n_above);
}

__global__ __launch_bounds__(TK_TILE_WAVES * 64) void topk_colmajor_kernel(const float* __restrict__ x, long long rows, int cols, long long col_stride,
                                                                           int k, float above, int* __restrict__ ids, float* __restrict__ vals,
                                                                           int* __restrict__ n_above) {
    __shared__ float tk_tile[TK_MAX_COLS * TK_TILE_PITCH];          // [cols][TK_TILE_PITCH]
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long long r0 = (long long)blockIdx.x * TK_TILE_ROWS;
    const int tr = lane & (TK_TILE_ROWS - 1), tc = lane / TK_TILE_ROWS;   // this lane's row and column of a wave-load: 4 columns x 16 rows
    const bool in_rows = r0 + tr < rows;
    // a wave's up to 4 loads are all issued before the first LDS write: one round trip to memory, not one per load
    float stage[TK_STAGE_LOADS];
#pragma unroll
    for (int i = 0; i < TK_STAGE_LOADS; ++i) {
        const int c = (i * TK_TILE_WAVES + w) * TK_COLS_PER_LOAD + tc;
        stage[i] = (c < cols && in_rows) ? x[(long long)c * col_stride + r0 + tr] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < TK_STAGE_LOADS; ++i) {
        const int c = (i * TK_TILE_WAVES + w) * TK_COLS_PER_LOAD + tc;
        if (c < cols) tk_tile[c * TK_TILE_PITCH + tr] = stage[i];
    }
    __syncthreads();
    float val[TK_ROWS_PER_WAVE][TK_SLOTS];
#pragma unroll
    for (int q = 0; q < TK_ROWS_PER_WAVE; ++q) {
#pragma unroll
        for (int s = 0; s < TK_SLOTS; ++s)
            val[q][s] = lane + 64 * s < cols ? tk_tile[(lane + 64 * s) * TK_TILE_PITCH + w * TK_ROWS_PER_WAVE + q] : 0.f;
    }
    float v[TK_ROWS_PER_WAVE];
    int c[TK_ROWS_PER_WAVE], n[TK_ROWS_PER_WAVE];
    tk_select<TK_ROWS_PER_WAVE>(val, cols, k, above, v, c, n);
#pragma unroll
    for (int q = 0; q < TK_ROWS_PER_WAVE; ++q) {
        const long long row = r0 + w * TK_ROWS_PER_WAVE + q;
        if (row < rows) tk_store(row, k, v[q], c[q], n[q], ids, vals, n_above);
    }
}

}  // namespace

extern "C" int mt4_topk_rows_f32(const float* x, int64_t rows, int32_t cols, int64_t row_stride, int64_t col_stride, int32_t k, float count_above,
                                 int32_t* ids, float* vals, int32_t* n_above, void* stream) {
    mt4_clear_error();
    if (!x || !ids || !vals || rows <= 0 || cols <= 0 || k <= 0 || row_stride <= 0 || col_stride <= 0) return MT4_EINVAL;
    if (cols > TK_MAX_COLS || k > TK_MAX_K || k > cols) return MT4_EUNSUPPORTED;
    const bool row_major = col_stride == 1 && (row_stride >= cols || rows == 1);
    const bool col_major = row_stride == 1 && (col_stride >= rows || cols == 1);
    if (!row_major && !col_major) return MT4_EUNSUPPORTED;         // a general strided gather: no form
    if (row_major) {
        const long long groups = ((long long)rows + 3) / 4;
        if (groups > 0x7FFFFFFFLL) return MT4_EUNSUPPORTED;
        hipLaunchKernelGGL(topk_rowmajor_kernel, dim3((unsigned)groups), dim3(256), 0, (hipStream_t)stream, x, (long long)rows, (int)cols,
                           (long long)row_stride, (int)k, count_above, (int*)ids, vals, (int*)n_above);
        return mt4_check_launch();
    }
    const long long tiles = ((long long)rows + TK_TILE_ROWS - 1) / TK_TILE_ROWS;
    if (tiles > 0x7FFFFFFFLL) return MT4_EUNSUPPORTED;
    static_assert(TK_MAX_COLS * TK_TILE_PITCH * 4 <= 64 * 1024 && TK_STAGE_LOADS * TK_TILE_WAVES * TK_COLS_PER_LOAD == TK_MAX_COLS, "the staged tile");
    hipLaunchKernelGGL(topk_colmajor_kernel, dim3((unsigned)tiles), dim3(TK_TILE_WAVES * 64), 0, (hipStream_t)stream, x, (long long)rows, (int)cols,
                       (long long)col_stride, (int)k, count_above, (int*)ids, vals, (int*)n_above);
    return mt4_check_launch();
}
