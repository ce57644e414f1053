// Image-quality metrics of the evaluators (gfx950): per image pair of NHWC uint8 images, the exact integer sums of (a-b)^2 and
// |a-b| and the mean of the reference's per-pixel SSIM (viewformer/utils/metrics.py:17-69 as SSIMMetric calls it, :177-184:
// K1 = 1, K2 = 0.03, data_range 1, 7x7 uniform window, VALID, sample covariance), in one pass over the bytes.
//
// Arithmetic.  On 0..255 values every 7x7 window sum of x, y, x^2, y^2 and xy is an integer below 49 * 255^2 = 3 186 225, so the
// box sums are int32 and the vertical sliding (add the new row, subtract the row seven above) is exact.  The reference's terms,
// scaled by (49 * 255)^2 (means) and 48 * 49 * 255^2 (covariances), become the integers
//     2 sx sy,  sx^2 + sy^2,  2 (49 sxy - sx sy),  (49 sxx - sx^2) + (49 syy - sy^2)      (all below 2^31)
// and only the per-pixel ratio  (2 sx sy + c1)(2 dxy + c2) / ((sx^2 + sy^2 + c1)(dxx + dyy + c2))  is floating point (fp64); an
// identical pair gives the same numerator and denominator, hence exactly 1.
//
// Layout.  One workgroup per (image, band of IM_BAND output rows, tile of IM_TJ output columns); a row is W*C flat bytes, so
// output column j (= x*C + c) is the stride-C 7-tap sum over input columns j .. j+6C.  The band plus its 6 halo rows (and the tile
// plus its 6C halo bytes) of both images is staged into LDS as (a | b << 8) pairs; each thread owns one output column and walks
// down the band keeping the seven last rows' horizontal sums in registers.  Per-workgroup partials go to the workspace and a
// second launch reduces them per image in a fixed order: no atomics, the same bits whatever the batch and from run to run.
#include "vf_common.h"
#include "../../include/vf_hip.h"

namespace {

constexpr int IM_THREADS = 256;
constexpr int IM_BAND = 32;                  // output rows per workgroup
constexpr int IM_TJ = IM_THREADS;            // output columns (flat x*C + c) per workgroup: one per thread
constexpr int IM_ROWS = IM_BAND + 6;         // staged input rows
constexpr int IM_COLS = IM_TJ + 6 * 4;       // staged input bytes per row (C <= 4)
constexpr int IM_C1S = 156125025;            // C1 = (K1 * 1)^2 = 1 scaled by (49 * 255)^2
constexpr double IM_C2S = 0.03 * 0.03 * 152938800.0;   // C2 = (0.03 * 1)^2 scaled by 48 * 49 * 255^2

struct ImPartial {
    long long sq, ab;
    double ssim;
};

__device__ __forceinline__ double im_ssim(int sx, int sy, int sxx, int syy, int sxy) {
    const int dxx = 49 * sxx - sx * sx, dyy = 49 * syy - sy * sy, dxy = 49 * sxy - sx * sy;
    const double a1 = (double)(2 * sx * sy + IM_C1S), b1 = (double)(sx * sx + sy * sy + IM_C1S);
    const double a2 = (double)(2 * dxy) + IM_C2S, b2 = (double)(dxx + dyy) + IM_C2S;
    return (a1 * a2) / (b1 * b2);
}

__global__ __launch_bounds__(IM_THREADS) void image_metrics_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                                  int H, int W, int C, int nbands, int ntiles,
                                                                  ImPartial* __restrict__ part) {
    __shared__ uint16_t tile[IM_ROWS][IM_COLS];
    __shared__ long long red_sq[IM_THREADS / VF_WAVE], red_ab[IM_THREADS / VF_WAVE];
    __shared__ double red_s[IM_THREADS / VF_WAVE];
    const int tid = threadIdx.x;
    const long long blk = blockIdx.x;
    const int t = (int)(blk % ntiles), band = (int)((blk / ntiles) % nbands);
    const long long img = blk / ((long long)ntiles * nbands);
    const int rowlen = W * C;
    const int r0 = band * IM_BAND, col0 = t * IM_TJ;
    const int nrows = min(IM_ROWS, H - r0), ncols = min(IM_TJ + 6 * C, rowlen - col0);
    // every input byte is counted by exactly one workgroup: its own band / tile, the last band / tile also takes the halo
    const int own_rows = band == nbands - 1 ? nrows : IM_BAND, own_cols = t == ntiles - 1 ? ncols : IM_TJ;
    const long long base = (img * H + r0) * (long long)rowlen + col0;
    const uint8_t* pa = a + base;
    const uint8_t* pb = b + base;
    int sq = 0, ab = 0;
    for (int r = 0; r < nrows; ++r)
        for (int c = tid; c < ncols; c += IM_THREADS) {
            const int x = pa[(long long)r * rowlen + c], y = pb[(long long)r * rowlen + c];
            tile[r][c] = (uint16_t)(x | (y << 8));
            if (r < own_rows && c < own_cols) {
                const int d = x - y;
                sq += d * d;
                ab += d < 0 ? -d : d;
            }
        }
    __syncthreads();

    const int out_rows = min(IM_BAND, H - 6 - r0), out_cols = min(IM_TJ, (W - 6) * C - col0);
    double acc = 0.0;
    if (tid < out_cols) {
        int hx[7], hy[7], hxx[7], hyy[7], hxy[7];     // horizontal sums of the last seven rows (slot = row % 7)
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
        const int in_rows = out_rows + 6;
        for (int rb = 0; rb < in_rows; rb += 7) {
#pragma unroll
            for (int k = 0; k < 7; ++k) {
                const int r = rb + k;
                if (r < in_rows) {
                    int ux = 0, uy = 0, uxx = 0, uyy = 0, uxy = 0;
#pragma unroll
                    for (int q = 0; q < 7; ++q) {
                        const int v = tile[r][tid + q * C];
                        const int x = v & 255, y = v >> 8;
                        ux += x;
                        uy += y;
                        uxx += x * x;
                        uyy += y * y;
                        uxy += x * y;
                    }
                    if (r >= 7) {
                        sx -= hx[k];
                        sy -= hy[k];
                        sxx -= hxx[k];
                        syy -= hyy[k];
                        sxy -= hxy[k];
                    }
                    hx[k] = ux;
                    hy[k] = uy;
                    hxx[k] = uxx;
                    hyy[k] = uyy;
                    hxy[k] = uxy;
                    sx += ux;
                    sy += uy;
                    sxx += uxx;
                    syy += uyy;
                    sxy += uxy;
                    if (r >= 6) acc += im_ssim(sx, sy, sxx, syy, sxy);
                }
            }
        }
    }

    // workgroup reduction in a fixed order: butterfly inside each wave, then the waves in index order
    long long lsq = sq, lab = ab;
#pragma unroll
    for (int o = VF_WAVE / 2; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o);
        lsq += __shfl_xor(lsq, o);
        lab += __shfl_xor(lab, o);
    }
    const int wave = tid / VF_WAVE;
    if ((tid & (VF_WAVE - 1)) == 0) {
        red_s[wave] = acc;
        red_sq[wave] = lsq;
        red_ab[wave] = lab;
    }
    __syncthreads();
    if (tid == 0) {
        ImPartial p = {0, 0, 0.0};
        for (int w = 0; w < IM_THREADS / VF_WAVE; ++w) {
            p.sq += red_sq[w];
            p.ab += red_ab[w];
            p.ssim += red_s[w];
        }
        part[blk] = p;
    }
}

// one thread per image: its workgroups' partials in index order
__global__ void image_metrics_finalize_kernel(const ImPartial* __restrict__ part, int nblk, int n_img, double count,
                                              long long* __restrict__ sums, double* __restrict__ ssim) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_img) return;
    long long sq = 0, ab = 0;
    double s = 0.0;
    for (int k = 0; k < nblk; ++k) {
        const ImPartial p = part[(long long)i * nblk + k];
        sq += p.sq;
        ab += p.ab;
        s += p.ssim;
    }
    sums[2 * (long long)i] = sq;
    sums[2 * (long long)i + 1] = ab;
    ssim[i] = s / count;
}

bool im_shape_ok(int n_img, int H, int W, int C) {
    return n_img >= 1 && H >= 7 && W >= 7 && C >= 1 && C <= 4 && (long long)W * C <= (1 << 30) && (long long)H * W * C <= (1ll << 40);
}

void im_grid(int H, int W, int C, int& nbands, int& ntiles) {
    nbands = (H - 6 + IM_BAND - 1) / IM_BAND;
    ntiles = ((W - 6) * C + IM_TJ - 1) / IM_TJ;
}

}  // namespace

extern "C" {

size_t vf_image_metrics_workspace_bytes(int n_img, int H, int W, int C) {
    if (!im_shape_ok(n_img, H, W, C)) return 0;
    int nbands, ntiles;
    im_grid(H, W, C, nbands, ntiles);
    return (size_t)n_img * nbands * ntiles * sizeof(ImPartial);
}

int vf_image_metrics_u8(const uint8_t* a, const uint8_t* b, int n_img, int H, int W, int C, int64_t* sums, double* ssim,
                        void* workspace, void* stream) {
    if (!a || !b || !sums || !ssim || !workspace || !im_shape_ok(n_img, H, W, C)) return VF_ERR_BAD_ARG;
    if (((uintptr_t)sums | (uintptr_t)ssim | (uintptr_t)workspace) & 7) return VF_ERR_BAD_ARG;
    int nbands, ntiles;
    im_grid(H, W, C, nbands, ntiles);
    const long long nblk = (long long)nbands * ntiles, blocks = nblk * n_img;
    if (blocks > 0x7fffffffll) return VF_ERR_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    ImPartial* part = (ImPartial*)workspace;
    hipLaunchKernelGGL(image_metrics_kernel, dim3((unsigned)blocks), dim3(IM_THREADS), 0, s, a, b, H, W, C, nbands, ntiles, part);
    const double count = (double)(H - 6) * (double)(W - 6) * (double)C;
    hipLaunchKernelGGL(image_metrics_finalize_kernel, dim3((unsigned)((n_img + 63) / 64)), dim3(64), 0, s, part, (int)nblk, n_img, count,
                       (long long*)sums, ssim);
    return vf_last_status();
}

}  // extern "C"
