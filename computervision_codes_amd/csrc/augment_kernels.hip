// The train transform of the frame trainers on the device (Spatial_cnn/dataloader.py:89-100,153-162): `Resize -> RandomVerticalFlip ->
// RandomHorizontalFlip -> RandomAutocontrast -> RandomRotation(expand) -> Resize` on uint8 frames, the same bytes as Pillow produces for the
// same random draws (augment.py draws them and builds the per-frame parameter table; its `reference_u8` is the same arithmetic in numpy).
//
//   mt4_aug_channel_luts      per frame and channel min / max -> the autocontrast lookup tables
//   mt4_aug_sharpen_u8        RandomAdjustSharpness(1.6) (the list's 'brightness') of the frames that drew it, a copy of the others
//   mt4_aug_flip_lut_rotate   flips + LUT + nearest-neighbour affine gather (16.16 fixed point) into a zero-filled padded canvas
//   mt4_aug_resize_pass_u8    mt4_resize_pass_u8 with per-frame input extents and per-frame coefficient tables out of a device pool
//
// The per-frame parameter row (int32 x MT4_AUG_PARAMS): {vflip, hflip, a0, a1, a2, a3, a4, a5, nw, nh, contrast, sharpen}; sharpen = 0 (not
// drawn), 1 (sharpen the frame as stored; an autocontrast, if drawn, follows and takes its range from the sharpened frame) or 2 (the frame's
// autocontrast comes first: the sharpening reads through the LUTs and mt4_aug_flip_lut_rotate does not apply them again).
#include "mt4_common.h"

// the autocontrast LUT is `int(i * scale + offset)` with TWO float64 roundings (Python floats): a fused multiply-add would change bytes
#pragma clang fp contract(off)

#define AUG_P MT4_AUG_PARAMS

// the kernels read and write dwords: every image, LUT and table pointer of the entry points must sit on a 4-byte boundary
static inline bool aug_dword_aligned(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// ------------------------------------------------------------------------------------------------ channel range + LUT
__global__ void aug_minmax_init_kernel(int* __restrict__ minmax, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) minmax[i] = (i & 1) ? 0 : 255;                  // [B][3][2] = (min, max)
}

// grid (blocks per frame, B).  A frame is n = H*W*3 bytes whose channel is (byte index % 3); a thread walks groups of 12 bytes (4 pixels, three
// dwords when the frame's bytes are dword-aligned), the wave folds with shuffles, the block through LDS, and six vector atomics per block
// reach the [B][3][2] table.  Frames without the autocontrast draw are skipped (their LUT is the identity).
__global__ void __launch_bounds__(256) aug_minmax_kernel(const uint8_t* __restrict__ frames, const int* __restrict__ params,
                                                         int* __restrict__ minmax, long long n) {
    const int b = blockIdx.y;
    if (!params[b * AUG_P + 10]) return;
    const uint8_t* f = frames + (long long)b * n;
    int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
    const long long groups = n / 12;
    const bool aligned = (n & 3) == 0;                         // then every frame starts on a dword (the entry point checks the base)
    for (long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (long long)gridDim.x * blockDim.x) {
        uint32_t w[3];
        if (aligned) {
            const uint32_t* p = (const uint32_t*)(f + g * 12);
            w[0] = p[0]; w[1] = p[1]; w[2] = p[2];
        } else {
            const uint8_t* p = f + g * 12;
#pragma unroll
            for (int k = 0; k < 3; ++k) w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        }
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            const int v = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
            lo[k % 3] = min(lo[k % 3], v);
            hi[k % 3] = max(hi[k % 3], v);
        }
    }
    if (blockIdx.x == 0) {                                     // the n % 12 bytes behind the last whole group (a multiple of 3)
        for (long long j = groups * 12 + threadIdx.x; j < n; j += blockDim.x) {
            const int v = f[j], c = (int)(j % 3);
            if (c == 0) { lo[0] = min(lo[0], v); hi[0] = max(hi[0], v); }
            else if (c == 1) { lo[1] = min(lo[1], v); hi[1] = max(hi[1], v); }
            else { lo[2] = min(lo[2], v); hi[2] = max(hi[2], v); }
        }
    }
    __shared__ int s[6];
    if (threadIdx.x < 6) s[threadIdx.x] = (threadIdx.x & 1) ? 0 : 255;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            lo[c] = min(lo[c], __shfl_xor(lo[c], off));
            hi[c] = max(hi[c], __shfl_xor(hi[c], off));
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            atomicMin(&s[2 * c], lo[c]);
            atomicMax(&s[2 * c + 1], hi[c]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        int* dst = minmax + b * 6 + threadIdx.x;
        if (threadIdx.x & 1) atomicMax(dst, s[threadIdx.x]);
        else atomicMin(dst, s[threadIdx.x]);
    }
}

// `ImageOps.autocontrast(im)` per channel: hi <= lo -> unchanged; else scale = 255.0 / (hi - lo), offset = -lo * scale (float64) and
// lut[i] = clamp(int(i * scale + offset), 0, 255), the product and the sum rounded separately (contraction is off in this file)
__global__ void aug_lut_kernel(const int* __restrict__ params, const int* __restrict__ minmax, uint8_t* __restrict__ luts, int B) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * 768) return;
    const int i = idx & 255, bc = idx >> 8, b = bc / 3;
    int v = i;
    if (params[b * AUG_P + 10]) {
        const int lo = minmax[2 * bc], hi = minmax[2 * bc + 1];
        if (hi > lo) {
            const double scale = 255.0 / (double)(hi - lo);
            const double offset = (double)(-lo) * scale;
            const double prod = (double)i * scale;
            const double t = prod + offset;
            v = (int)t;                                        // truncation toward zero, as Python's int()
            v = v < 0 ? 0 : (v > 255 ? 255 : v);
        }
    }
    luts[idx] = (uint8_t)v;
}

extern "C" int mt4_aug_channel_luts(const uint8_t* frames, const int32_t* params, int32_t* minmax, uint8_t* luts, int32_t B, int32_t H,
                                    int32_t W, void* stream) {
    mt4_clear_error();
    if (!frames || !params || !minmax || !luts || B <= 0 || H <= 0 || W <= 0 || B > 65535) return MT4_EINVAL;
    if (!aug_dword_aligned(frames) || !aug_dword_aligned(luts)) return MT4_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const long long n = (long long)H * W * 3;
    hipLaunchKernelGGL(aug_minmax_init_kernel, dim3(cdiv(B * 6, 256)), dim3(256), 0, s, minmax, B * 6);
    const long long groups = n / 12;
    int blocks = (int)((groups + 256 * 4 - 1) / (256 * 4));   // four groups (48 bytes) per thread
    blocks = blocks < 1 ? 1 : (blocks > 64 ? 64 : blocks);
    hipLaunchKernelGGL(aug_minmax_kernel, dim3(blocks, B), dim3(256), 0, s, frames, params, minmax, n);
    hipLaunchKernelGGL(aug_lut_kernel, dim3(cdiv(B * 768, 256)), dim3(256), 0, s, params, minmax, luts, B);
    return mt4_check_launch();
}

// ------------------------------------------------------------------------------------------------ sharpening ('brightness')
// `ImageEnhance.Sharpness(im).enhance(1.6)` = blend(im.filter(SMOOTH), im, 1.6) in integers.  With N = the sum of the 3 x 3 neighbourhood plus
// 4 x the centre (SMOOTH is [1 1 1; 1 5 1; 1 1 1] / 13), Pillow's float32 `0.5 + N / 13` truncated is deg = (2 N + 13) / 26: 13 is odd, so the
// float sum is never within 1/26 of an integer.  The blend p + 0.6 (p - deg), truncated toward zero and clamped, is (5 deg + 8 (p - deg)) / 5
// with C's division.  The one-pixel border of the image is the source, so an image with H < 3 or W < 3 is all border and comes back unchanged
// (through its LUTs when they come first).  Nothing of this depends on the float unit.
#define AUG_SH_ROWS 16                                         // a workgroup's tile: 16 rows x 64 pixels, a thread = 4 adjacent pixels of one row
#define AUG_SH_COLS 64
// LDS image of the tile: AUG_SH_ROWS + 2 rows of the bytes [3 X0 - 4, 3 X0 + 200) of the frame's row = 51 dwords, the dword that holds the left
// halo pixel first.  A thread reads dwords 3 tx .. 3 tx + 4 of three rows; with a row stride of 16 mod 32 dwords the two rows of a 32-lane group
// fall on disjoint banks ({3 t mod 32, t < 16} and the same set + 16).  Not measured against the dense stride.
#define AUG_SH_STRIDE 80

__device__ __forceinline__ uint32_t aug_sharpen_byte(int n, int p) {
    const int deg = (2 * n + 13) / 26;
    const int t = (5 * deg + 8 * (p - deg)) / 5;               // (truncation toward zero, as the float-to-int conversion of the blend)
    return (uint32_t)(t < 0 ? 0 : (t > 255 ? 255 : t));
}

// grid (ceil(W / 64), ceil(H / 16), B).  mode = params[b][11]: 0 -> the tile is copied; 1, 2 -> sharpened, through the frame's LUTs when mode == 2
// and luts != NULL.  Any other value sharpens like 1 (`augment.draw_params` writes 0, 1 or 2; the rows live on the device, so the entry point
// cannot refuse them).  Rows are read and written as dwords when W % 4 == 0 (then every row of every frame starts on a dword), byte by byte
// otherwise.
__global__ void __launch_bounds__(256) aug_sharpen_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ luts,
                                                          const int* __restrict__ params, uint8_t* __restrict__ out, int H, int W) {
    __shared__ uint32_t simg[(AUG_SH_ROWS + 2) * AUG_SH_STRIDE];
    __shared__ uint32_t slut32[192];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int mode = params[b * AUG_P + 11];
    const int X0 = blockIdx.x * AUG_SH_COLS, Y0 = blockIdx.y * AUG_SH_ROWS;
    const int tx = tid & 15, ty = tid >> 4;
    const int X = X0 + tx * 4, Y = Y0 + ty;
    const int rowb = W * 3;
    const bool aligned = (W & 3) == 0;
    const uint8_t* f = frames + (long long)b * H * rowb;
    uint8_t* dst = out + ((long long)b * H + Y) * rowb + X * 3;
    if (mode == 0) {                                           // (uniform over the workgroup: before any barrier)
        if (Y >= H || X >= W) return;
        const uint8_t* src = f + (long long)Y * rowb + X * 3;
        if (aligned) {
#pragma unroll
            for (int k = 0; k < 3; ++k) ((uint32_t*)dst)[k] = ((const uint32_t*)src)[k];
        } else {
            for (int k = 0; k < 12; ++k)
                if (X + k / 3 < W) dst[k] = src[k];
        }
        return;
    }
    const bool use_lut = mode == 2 && luts != nullptr;
    if (use_lut && tid < 192) slut32[tid] = ((const uint32_t*)(luts + (long long)b * 768))[tid];
    if (use_lut) __syncthreads();
    const uint8_t* slut = (const uint8_t*)slut32;
    // stage: LDS byte j of LDS row r is byte 3 X0 - 4 + j of frame row Y0 - 1 + r.  Bytes outside the frame are staged as 0 (as lut[0] inside
    // the frame's rows when the LUTs apply); their value is never used: only border pixels, which are copies, have such neighbours
    for (int i = tid; i < (AUG_SH_ROWS + 2) * 51; i += 256) {
        const int r = i / 51, k = i - r * 51;
        const int y = Y0 - 1 + r, g0 = X0 * 3 - 4 + 4 * k;
        uint32_t v = 0;
        if (y >= 0 && y < H) {
            const uint8_t* row = f + (long long)y * rowb;
            if (aligned) {
                if (g0 >= 0 && g0 < rowb) v = *(const uint32_t*)(row + g0);      // (rowb % 4 == 0: a dword is inside or outside as a whole)
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (g0 + e >= 0 && g0 + e < rowb) v |= (uint32_t)row[g0 + e] << (8 * e);
            }
            if (use_lut) {                                     // the channel of row byte g is g % 3, and 3 X0 - 4 = 2 (mod 3)
                uint32_t t = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) t |= (uint32_t)slut[((4 * k + e + 2) % 3) * 256 + ((v >> (8 * e)) & 255u)] << (8 * e);
                v = t;
            }
        }
        simg[r * AUG_SH_STRIDE + k] = v;
    }
    __syncthreads();
    if (Y >= H || X >= W) return;
    // bytes 12 tx .. 12 tx + 19 of the rows above, at and below: output byte k of the thread is LDS byte 4 + k, its left and right neighbours
    // (the same channel of the adjacent pixels) bytes 1 + k and 7 + k
    uint32_t d[3][5];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 5; ++q) d[r][q] = simg[(ty + r) * AUG_SH_STRIDE + 3 * tx + q];
    int mid[20], col[20];
#pragma unroll
    for (int j = 1; j < 19; ++j) {
        const int sh = 8 * (j & 3);
        mid[j] = (int)((d[1][j >> 2] >> sh) & 255u);
        col[j] = (int)((d[0][j >> 2] >> sh) & 255u) + mid[j] + (int)((d[2][j >> 2] >> sh) & 255u);
    }
    const bool yedge = Y == 0 || Y == H - 1;
    uint32_t px[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        const int x = X + k / 3, p = mid[4 + k];
        const bool edge = yedge || x == 0 || x >= W - 1;
        px[k] = edge ? (uint32_t)p : aug_sharpen_byte(col[1 + k] + col[4 + k] + col[7 + k] + 4 * p, p);
    }
    if (aligned) {                                             // X % 4 == 0 and W % 4 == 0: all four pixels inside, 12-byte aligned
        uint32_t* o = (uint32_t*)dst;
#pragma unroll
        for (int k = 0; k < 3; ++k) o[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | (px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 12; ++k)
            if (X + k / 3 < W) dst[k] = (uint8_t)px[k];
    }
}

extern "C" int mt4_aug_sharpen_u8(const uint8_t* frames, const uint8_t* luts, const int32_t* params, uint8_t* out, int32_t B, int32_t H,
                                  int32_t W, void* stream) {
    mt4_clear_error();
    if (!frames || !params || !out || frames == out || B <= 0 || H <= 0 || W <= 0) return MT4_EINVAL;
    if (B > 65535 || H > 4096 || W > 4096) return MT4_EINVAL;
    if (!aug_dword_aligned(frames) || !aug_dword_aligned(out) || !aug_dword_aligned(luts)) return MT4_EINVAL;
    hipLaunchKernelGGL(aug_sharpen_kernel, dim3(cdiv(W, AUG_SH_COLS), cdiv(H, AUG_SH_ROWS), B), dim3(256), 0, (hipStream_t)stream, frames, luts,
                       params, out, H, W);
    return mt4_check_launch();
}

// ------------------------------------------------------------------------------------------------ flips + LUT + rotation gather
// Output pixel (X, Y) of frame b, X < nw and Y < nh, reads source pixel xin = (a2 + X a0 + Y a1) >> 16, yin = (a5 + X a3 + Y a4) >> 16
// (arithmetic shift; Pillow's affine transform with the NEAREST filter) of the flipped frame, i.e. (W-1-xin if hflip, H-1-yin if vflip) of the
// frame as stored, through the channel's LUT (not for a frame whose row says that mt4_aug_sharpen_u8 applied it: sharpen == 2); 0 outside the source, and 0 in the canvas outside nw x nh.  A workgroup writes a 64 x 16 pixel
// tile, so its source footprint is the rotated 64 x 16 rectangle; a thread writes 4 adjacent pixels = 12 bytes as three dwords when the canvas
// rows are dword-aligned (Wc % 4 == 0).
__global__ void __launch_bounds__(256) aug_flip_lut_rotate_kernel(const uint8_t* __restrict__ frames, const uint8_t* __restrict__ luts,
                                                                  const int* __restrict__ params, uint8_t* __restrict__ canvas, int H, int W,
                                                                  int Hc, int Wc) {
    __shared__ uint32_t slut32[192];
    const int b = blockIdx.z, tid = threadIdx.x;
    if (tid < 192) {                                           // (the load does not wait for the row: sharpen == 2 replaces what it brought)
        uint32_t v = ((const uint32_t*)(luts + (long long)b * 768))[tid];
        if (params[b * AUG_P + 11] == 2) v = 0x03020100u + (uint32_t)(tid & 63) * 0x04040404u;      // the identity table: bytes 4 i .. 4 i + 3
        slut32[tid] = v;
    }
    __syncthreads();
    const uint8_t* slut = (const uint8_t*)slut32;
    const int X0 = blockIdx.x * 64 + (tid & 15) * 4, Y = blockIdx.y * 16 + (tid >> 4);
    if (Y >= Hc || X0 >= Wc) return;
    const int* p = params + b * AUG_P;
    const int vflip = p[0], hflip = p[1], a0 = p[2], a1 = p[3], a2 = p[4], a3 = p[5], a4 = p[6], a5 = p[7], nw = p[8], nh = p[9];
    const uint8_t* f = frames + (long long)b * H * W * 3;
    uint32_t px[12];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int X = X0 + e;
        uint32_t r = 0, g = 0, bl = 0;
        if (X < nw && Y < nh) {
            const int xin = (a2 + X * a0 + Y * a1) >> 16, yin = (a5 + X * a3 + Y * a4) >> 16;
            if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
                const int xs = hflip ? W - 1 - xin : xin, ys = vflip ? H - 1 - yin : yin;
                const uint8_t* src = f + ((long long)ys * W + xs) * 3;
                r = slut[src[0]]; g = slut[256 + src[1]]; bl = slut[512 + src[2]];
            }
        }
        px[3 * e] = r; px[3 * e + 1] = g; px[3 * e + 2] = bl;
    }
    uint8_t* dst = canvas + (((long long)b * Hc + Y) * Wc + X0) * 3;
    if ((Wc & 3) == 0) {                                       // X0 % 4 == 0 and Wc % 4 == 0: all four pixels inside, 12-byte aligned
        uint32_t* d = (uint32_t*)dst;
#pragma unroll
        for (int k = 0; k < 3; ++k) d[k] = px[4 * k] | (px[4 * k + 1] << 8) | (px[4 * k + 2] << 16) | (px[4 * k + 3] << 24);
    } else {
        for (int k = 0; k < 12; ++k)
            if (X0 + k / 3 < Wc) dst[k] = (uint8_t)px[k];
    }
}

extern "C" int mt4_aug_flip_lut_rotate(const uint8_t* frames, const uint8_t* luts, const int32_t* params, uint8_t* canvas, int32_t B,
                                       int32_t H, int32_t W, int32_t Hc, int32_t Wc, void* stream) {
    mt4_clear_error();
    if (!frames || !luts || !params || !canvas || B <= 0 || H <= 0 || W <= 0 || Hc <= 0 || Wc <= 0) return MT4_EINVAL;
    // |a0|, |a1|, |a3|, |a4| <= 65536 (a rotation) and X, Y < 8192, so |X a0 + Y a1| < 2^30; the offsets a2, a5 are source coordinates of the
    // canvas corner in 16.16, |a2|, |a5| < (4096 + 8192) * 65536 < 2^30 for a table of `draw_params` at these sizes: the sums stay inside int32
    if (B > 65535 || H > 4096 || W > 4096 || Hc > 8192 || Wc > 8192) return MT4_EINVAL;
    if (!aug_dword_aligned(luts) || !aug_dword_aligned(canvas)) return MT4_EINVAL;
    hipLaunchKernelGGL(aug_flip_lut_rotate_kernel, dim3(cdiv(Wc, 64), cdiv(Hc, 16), B), dim3(256), 0, (hipStream_t)stream, frames, luts, params,
                       canvas, H, W, Hc, Wc);
    return mt4_check_launch();
}

// ------------------------------------------------------------------------------------------------ resize passes, per-frame extents and tables
// Same arithmetic as resize_pass_u8_kernel (misc_kernels.hip): out = clip8((2^21 + sum_i in[lo + i] * kk[i]) >> 22).  Frame b's image is the
// top-left nh x nw corner of its canvas; its tables lie in `pool` (int32) at the offsets of its row of frame_tab:
//     {h bounds offset, h coeffs offset, h ksize, nw,  v bounds offset, v coeffs offset, v ksize, nh}
// (bounds [n_out][2] = (lo, count), coeffs [n_out][ksize]).  C = 3.
__device__ __forceinline__ uint32_t clip8(int ss) {
    ss >>= 22;
    return (uint32_t)(ss < 0 ? 0 : (ss > 255 ? 255 : ss));
}

#define AUG_HROWS 4                                            // rows staged in LDS at a time
#ifndef AUG_HGROUPS
// groups of AUG_HROWS rows a workgroup walks with one staged table.  Measured on the MI355X (batch 64 at 256 x 448 / batch 16 at 384 x 384, us per
// launch): 1 -> 73 / 27, 2 -> 67 / 29, 4 -> 77 / 40, 8 -> 106 / 68.  The table comes out of L2 and is cheap; a longer walk serialises a
// workgroup's load -> barrier -> compute rounds and leaves fewer workgroups to hide them behind.
#define AUG_HGROUPS 2
#endif
// AUG_HROWS staged rows -> their output rows, a dword = 4 adjacent bytes per thread and step.  `kt` is the frame's coefficient table: in LDS when
// it fits the launch's ksize_max, else the pool itself (the caller branches, so each instance keeps its address space).
__device__ __forceinline__ void aug_resize_h_rows(const uint8_t* srow, const int* sb, const int* kt, int ks, uint8_t* out_rows, int rows, int Wc,
                                                  int Wout, int win, int tid) {
    const int ob = Wout * 3, ipr = (ob + 3) / 4;
    const bool aligned = (ob & 3) == 0;
    for (int item = tid; item < rows * ipr; item += 256) {
        const int r = item / ipr, q = item - r * ipr;
        const uint8_t* row = srow + r * Wc * 3;
        uint32_t v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = q * 4 + e;
            v[e] = 0;
            if (j < ob) {
                const int o = j / 3, c = j - 3 * o;
                const int lo = sb[2 * o], n = min(sb[2 * o + 1], win - lo);
                const int* k = kt + o * ks;
                int ss = 1 << 21;
                for (int i = 0; i < n; ++i) ss += (int)row[(lo + i) * 3 + c] * k[i];
                v[e] = clip8(ss);
            }
        }
        uint8_t* dst = out_rows + (long long)r * ob + q * 4;
        if (aligned) *(uint32_t*)dst = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
        else
            for (int e = 0; e < 4; ++e)
                if (q * 4 + e < ob) dst[e] = (uint8_t)v[e];
    }
}

// axis 0: [B][Hc][Wc][3] -> [B][Hc][Wout][3], rows >= nh are left unwritten (the vertical pass never reads them).  grid (ceil(Hc / 8), B):
// the frame's whole horizontal table is staged in LDS once per workgroup and serves AUG_HGROUPS groups of four input rows (dword loads into
// LDS); every thread produces output dwords = 4 adjacent bytes of a row.
__global__ void __launch_bounds__(256) aug_resize_h_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int* __restrict__ pool,
                                                           const int* __restrict__ frame_tab, int Hc, int Wc, int Wout, int ksize_max) {
    extern __shared__ int smem[];
    int* sb = smem;                                            // [Wout][2]
    int* sk = smem + 2 * Wout;                                 // [Wout][ks]
    uint8_t* srow = (uint8_t*)(sk + Wout * ksize_max);         // [AUG_HROWS][Wc * 3]
    const int b = blockIdx.y, tid = threadIdx.x;
    const int* ft = frame_tab + b * 8;
    const int ks = ft[2], win = ft[3], nh = ft[7];
    const int y_first = blockIdx.x * (AUG_HROWS * AUG_HGROUPS);
    if (y_first >= nh) return;                                 // (uniform: before any barrier)
    const int* gb = pool + ft[0];
    const int* gk = pool + ft[1];
    const bool in_lds = ks <= ksize_max;                       // a frame whose table is wider than the launch sized LDS for reads the pool
    for (int i = tid; i < 2 * Wout; i += 256) sb[i] = gb[i];
    if (in_lds)
        for (int i = tid; i < Wout * ks; i += 256) sk[i] = gk[i];
    const int rowdw = Wc * 3 / 4;                              // Wc % 4 == 0 (checked by the entry point)
    const int y_end = min(nh, y_first + AUG_HROWS * AUG_HGROUPS);
    for (int y0 = y_first; y0 < y_end; y0 += AUG_HROWS) {      // (uniform trip count)
        const int rows = min(AUG_HROWS, y_end - y0);
        const uint32_t* in32 = (const uint32_t*)in + ((long long)b * Hc + y0) * rowdw;
        for (int i = tid; i < rows * rowdw; i += 256) ((uint32_t*)srow)[i] = in32[i];
        __syncthreads();
        uint8_t* out_rows = out + ((long long)b * Hc + y0) * Wout * 3;
        if (in_lds) aug_resize_h_rows(srow, sb, sk, ks, out_rows, rows, Wc, Wout, win, tid);
        else aug_resize_h_rows(srow, sb, gk, ks, out_rows, rows, Wc, Wout, win, tid);
        __syncthreads();                                       // srow is staged again
    }
}

// axis 1: [B][Hc][Wout][3] (rows < nh) -> [B][Hout][Wout][3].  grid (Hout, B): one output row per workgroup, so the row's (lo, count, kk[])
// are uniform and come through the scalar cache; a thread reads one dword of each contributing input row and writes one dword.
__global__ void __launch_bounds__(128) aug_resize_v_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int* __restrict__ pool,
                                                           const int* __restrict__ frame_tab, int Hc, int Hout, int Wout) {
    const int b = blockIdx.y, y = blockIdx.x;
    const int* ft = frame_tab + b * 8;
    const int ks = ft[6], nh = ft[7];
    const int lo = pool[ft[4] + 2 * y], n = min(pool[ft[4] + 2 * y + 1], nh - lo);
    const int* k = pool + ft[5] + (long long)y * ks;
    const int ob = Wout * 3;
    const uint8_t* src = in + ((long long)b * Hc + lo) * ob;
    uint8_t* dst = out + ((long long)b * Hout + y) * ob;
    if ((ob & 3) == 0) {
        const int rowdw = ob / 4;
        for (int q = threadIdx.x; q < rowdw; q += blockDim.x) {
            int acc[4] = {1 << 21, 1 << 21, 1 << 21, 1 << 21};
            for (int i = 0; i < n; ++i) {
                const uint32_t w = ((const uint32_t*)src)[(long long)i * rowdw + q];
                const int ki = k[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] += (int)((w >> (8 * e)) & 255u) * ki;
            }
            ((uint32_t*)dst)[q] = clip8(acc[0]) | (clip8(acc[1]) << 8) | (clip8(acc[2]) << 16) | (clip8(acc[3]) << 24);
        }
    } else {
        for (int j = threadIdx.x; j < ob; j += blockDim.x) {
            int ss = 1 << 21;
            for (int i = 0; i < n; ++i) ss += (int)src[(long long)i * ob + j] * k[i];
            dst[j] = (uint8_t)clip8(ss);
        }
    }
}

extern "C" int mt4_aug_resize_pass_u8(const uint8_t* in, uint8_t* out, const int32_t* pool, const int32_t* frame_tab, int32_t B, int32_t Hc,
                                      int32_t Wc, int32_t Hout, int32_t Wout, int32_t ksize_max, int32_t axis, void* stream) {
    mt4_clear_error();
    if (!in || !out || !pool || !frame_tab || B <= 0 || Hc <= 0 || Wc <= 0 || Hout <= 0 || Wout <= 0 || ksize_max <= 0 || B > 65535)
        return MT4_EINVAL;
    if (!aug_dword_aligned(in) || !aug_dword_aligned(out)) return MT4_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    if (axis == 0) {
        if (Hout != Hc || (Wc & 3)) return MT4_EINVAL;
        const long long lds = ((long long)Wout * (2 + ksize_max)) * 4 + (long long)AUG_HROWS * Wc * 3;
        if (lds > 64 * 1024) return MT4_EUNSUPPORTED;
        hipLaunchKernelGGL(aug_resize_h_kernel, dim3(cdiv(Hc, AUG_HROWS * AUG_HGROUPS), B), dim3(256), (size_t)lds, s, in, out, pool, frame_tab, Hc, Wc, Wout,
                           ksize_max);
    } else if (axis == 1) {
        if (Wc != Wout || Hout > 65535) return MT4_EINVAL;
        hipLaunchKernelGGL(aug_resize_v_kernel, dim3(Hout, B), dim3(128), 0, s, in, out, pool, frame_tab, Hc, Hout, Wout);
    } else {
        return MT4_EINVAL;
    }
    return mt4_check_launch();
}
