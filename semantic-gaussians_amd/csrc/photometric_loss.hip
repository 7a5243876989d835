// The training loss of train.py:138-150 as two kernels per direction:  (1 - lambda) * L1 + lambda * (1 - SSIM(image, gt)),
// SSIM as utils/loss_utils.py builds it (11-tap Gaussian window, sigma 1.5, zero padding of 5, C1 = 0.01^2, C2 = 0.03^2),
// forward and backward, on images given by base pointer + pitches.
//
// One workgroup of 256 threads owns one 32x32 tile of one (image, channel) plane.  The window is separable, so a tile is
// filtered in two passes through LDS: the 42x42 halo of the inputs is loaded once (zero outside the image: that IS the
// reference's padding), every thread filters a strip of 4 neighbouring columns of one halo row horizontally (14 LDS reads feed
// 4 x 11 taps), the 42x32 row sums go back to LDS, and every thread then filters 4 neighbouring rows of one column
// vertically the same way.  Row strides of 43 and 33 floats keep both passes free of bank conflicts (a strip start is a
// multiple of 4 floats: consecutive rows have to land on the banks in between).
//
// No floating-point atomics: every tile stores its two sums (SSIM, |x - y|) as doubles at its own position and
// loss_finish_kernel adds them in a fixed order, so a loss is the same bits on every run.
#include "sgs_kernels.h"

namespace sgs {

namespace {

constexpr int TS = 32;             // tile side (outputs)
constexpr int RAD = 5;             // window radius
constexpr int HS = TS + 2 * RAD;   // halo side, 42
constexpr int IN_LD = 43;          // row stride of a halo tile in LDS
constexpr int H_LD = 33;           // row stride of the row-filtered tile in LDS
constexpr int NT = 256;

// w: the 11 taps.  mass: what the reference's window sums to over what the separable one sums to, minus 1.  The reference filters with
// the 11x11 window whose entries are the FLOAT32-ROUNDED products w[i] * w[j]; rows-then-columns filters with the exact products.  The
// two differ by ~1e-8 in total mass, and sigma = E[x^2] - mu^2 turns a mass error d into -d * mu^2, which against sigma ~ 1e-3 and with
// one sign over the whole image moves the mean SSIM by 5e-7 -- several times the reference's own float32 error at 968x1296.  The
// first-order term of that mass difference is added to the three sigmas; what is left is 1e-10.
struct LossTaps { float w[2 * RAD + 1]; float mass; };

// halo tile of one plane into LDS, zero outside the image
__device__ __forceinline__ void load_halo(float* __restrict__ dst, const float* __restrict__ plane, long long row_pitch,
					  int H, int W, int y0, int x0)
{
	for (int i = threadIdx.x; i < HS * HS; i += NT) {
		const int r = i / HS, c = i - r * HS;
		const int gy = y0 - RAD + r, gx = x0 - RAD + c;
		float v = 0.f;
		if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = plane[(long long)gy * row_pitch + gx];
		dst[r * IN_LD + c] = v;
	}
}

// 14 consecutive floats of an LDS row -> 4 neighbouring 11-tap sums, taps applied in index order
__device__ __forceinline__ void taps4(const float (&v)[14], const LossTaps& t, float (&out)[4])
{
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		float s = v[j] * t.w[0];
#pragma unroll
		for (int k = 1; k < 11; ++k) s = fmaf(v[j + k], t.w[k], s);
		out[j] = s;
	}
}

// column `c`, rows r0 .. r0+3 of one row-filtered quantity
__device__ __forceinline__ void vertical4(const float* __restrict__ h, int c, int r0, const LossTaps& t, float (&out)[4])
{
	float v[14];
#pragma unroll
	for (int k = 0; k < 14; ++k) v[k] = h[(r0 + k) * H_LD + c];
	taps4(v, t, out);
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	return v;
}

// SSIM: with the SSIM term (else L1 only).  MAPS: store the three derivative maps the backward filters.
template <bool SSIM, bool MAPS>
__global__ __launch_bounds__(NT) void loss_forward_kernel(int C, int H, int W, const float* __restrict__ img, long long img_row,
							   long long img_ch, long long img_im, const float* __restrict__ gt,
							   long long gt_row, long long gt_ch, long long gt_im, LossTaps taps,
							   float* __restrict__ dmaps, long long map_stride, double* __restrict__ partials)
{
	__shared__ float s_x[HS * IN_LD];
	__shared__ float s_y[HS * IN_LD];
	__shared__ float s_h[SSIM ? 5 * HS * H_LD : 1];
	__shared__ double s_red[2 * (NT / 64)];

	const int plane = blockIdx.z, b = plane / C, ch = plane - b * C;
	const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
	const float* px = img + (long long)b * img_im + (long long)ch * img_ch;
	const float* py = gt + (long long)b * gt_im + (long long)ch * gt_ch;
	load_halo(s_x, px, img_row, H, W, y0, x0);
	load_halo(s_y, py, gt_row, H, W, y0, x0);
	__syncthreads();

	if (SSIM) {
		// rows: 42 halo rows x 8 strips of 4 columns
		for (int i = threadIdx.x; i < HS * (TS / 4); i += NT) {
			const int r = i >> 3, c0 = (i & 7) * 4;
			float x[14], y[14], q[14], o[4];
#pragma unroll
			for (int k = 0; k < 14; ++k) {
				x[k] = s_x[r * IN_LD + c0 + k];
				y[k] = s_y[r * IN_LD + c0 + k];
			}
			float* h = s_h + r * H_LD + c0;
			taps4(x, taps, o);
#pragma unroll
			for (int j = 0; j < 4; ++j) h[0 * HS * H_LD + j] = o[j];
			taps4(y, taps, o);
#pragma unroll
			for (int j = 0; j < 4; ++j) h[1 * HS * H_LD + j] = o[j];
#pragma unroll
			for (int k = 0; k < 14; ++k) q[k] = x[k] * x[k];
			taps4(q, taps, o);
#pragma unroll
			for (int j = 0; j < 4; ++j) h[2 * HS * H_LD + j] = o[j];
#pragma unroll
			for (int k = 0; k < 14; ++k) q[k] = y[k] * y[k];
			taps4(q, taps, o);
#pragma unroll
			for (int j = 0; j < 4; ++j) h[3 * HS * H_LD + j] = o[j];
#pragma unroll
			for (int k = 0; k < 14; ++k) q[k] = x[k] * y[k];
			taps4(q, taps, o);
#pragma unroll
			for (int j = 0; j < 4; ++j) h[4 * HS * H_LD + j] = o[j];
		}
		__syncthreads();
	}

	// columns: thread = (column, group of 4 rows)
	const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
	const int gx = x0 + c;
	float mu1[4], mu2[4], exx[4], eyy[4], exy[4];
	if (SSIM) {
		vertical4(s_h + 0 * HS * H_LD, c, r0, taps, mu1);
		vertical4(s_h + 1 * HS * H_LD, c, r0, taps, mu2);
		vertical4(s_h + 2 * HS * H_LD, c, r0, taps, exx);
		vertical4(s_h + 3 * HS * H_LD, c, r0, taps, eyy);
		vertical4(s_h + 4 * HS * H_LD, c, r0, taps, exy);
	}
	const float C1 = 0.0001f, C2 = 0.0009f;
	double sum_ssim = 0.0, sum_l1 = 0.0;
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const int gy = y0 + r0 + j;
		if (gy >= H || gx >= W) continue;
		const float x = s_x[(r0 + j + RAD) * IN_LD + c + RAD], y = s_y[(r0 + j + RAD) * IN_LD + c + RAD];
		sum_l1 += (double)fabsf(x - y);
		if (SSIM) {
			// utils/loss_utils.py:53-64, operation for operation (plus the window's mass term, LossTaps)
			const float m1 = mu1[j], m2 = mu2[j];
			const float m1s = m1 * m1, m2s = m2 * m2, m12 = m1 * m2;
			float s1 = exx[j] - m1s, s2 = eyy[j] - m2s, s12 = exy[j] - m12;
			s1 = fmaf(taps.mass, exx[j] - 2.f * m1s, s1);
			s2 = fmaf(taps.mass, eyy[j] - 2.f * m2s, s2);
			s12 = fmaf(taps.mass, exy[j] - 2.f * m12, s12);
			const float A1 = 2.f * m12 + C1, A2 = 2.f * s12 + C2;
			const float B1 = m1s + m2s + C1, B2 = s1 + s2 + C2;
			const float inv = 1.f / (B1 * B2);
			sum_ssim += (double)((A1 * A2) / (B1 * B2));
			if (MAPS) {
				// partial derivatives of the map value by mu1, sigma1^2 and sigma12; the mean's own entry also takes what
				// reaches it through sigma1^2 = E[x^2] - mu1^2 and sigma12 = E[xy] - mu1 mu2.  Deliberately taken as if the
				// mass term above were absent: it would change these maps by a factor 1 + O(mass), ~1e-8 relative, far under fp32 rounding
				const float d_s1 = -(A1 * A2) * inv / B2;
				const float d_s12 = 2.f * A1 * inv;
				const float d_m1 = 2.f * m2 * A2 * inv - 2.f * m1 * (A1 * A2) * inv / B1;
				const long long at = (long long)plane * H * W + (long long)gy * W + gx;
				dmaps[at] = d_m1 - 2.f * m1 * d_s1 - m2 * d_s12;
				dmaps[map_stride + at] = d_s1;
				dmaps[2 * map_stride + at] = d_s12;
			}
		}
	}
	sum_ssim = wave_sum(sum_ssim);
	sum_l1 = wave_sum(sum_l1);
	const int wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) {
		s_red[2 * wave] = sum_ssim;
		s_red[2 * wave + 1] = sum_l1;
	}
	__syncthreads();
	if (threadIdx.x == 0) {
		double a = 0.0, l = 0.0;
		for (int w = 0; w < NT / 64; ++w) {
			a += s_red[2 * w];
			l += s_red[2 * w + 1];
		}
		const long long tile = ((long long)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
		partials[2 * tile] = a;
		partials[2 * tile + 1] = l;
	}
}

// one workgroup per output entry: the tiles' sums in a fixed order, in double
__global__ __launch_bounds__(NT) void loss_finish_kernel(const double* __restrict__ partials, long long tiles_per_out, double count,
							  float lambda, float* __restrict__ out_loss, float* __restrict__ out_ssim,
							  float* __restrict__ out_l1)
{
	__shared__ double s_a[NT], s_l[NT];
	const double* p = partials + 2 * tiles_per_out * blockIdx.x;
	double a = 0.0, l = 0.0;
	for (long long i = threadIdx.x; i < tiles_per_out; i += NT) {
		a += p[2 * i];
		l += p[2 * i + 1];
	}
	s_a[threadIdx.x] = a;
	s_l[threadIdx.x] = l;
	__syncthreads();
	for (int o = NT / 2; o > 0; o >>= 1) {
		if ((int)threadIdx.x < o) {
			s_a[threadIdx.x] += s_a[threadIdx.x + o];
			s_l[threadIdx.x] += s_l[threadIdx.x + o];
		}
		__syncthreads();
	}
	if (threadIdx.x == 0) {
		const double ssim = s_a[0] / count, l1 = s_l[0] / count;
		if (out_ssim) out_ssim[blockIdx.x] = (float)ssim;
		if (out_l1) out_l1[blockIdx.x] = (float)l1;
		// lambda == 0 is the L1-only form: no SSIM was summed
		const double lam = (double)lambda;
		out_loss[blockIdx.x] = (float)(lambda == 0.f ? l1 : (1.0 - lam) * l1 + lam * (1.0 - ssim));
	}
}

// dL/dx = (g * w_ssim / N) * (F(dmu1) + 2 x F(dsigma1^2) + y F(dsigma12)) + (g * w_l1 / N) * sign(x - y)
// (the two factors rounded in the order autograd rounds them: the weight times the upstream gradient first, then the mean's 1/N)
template <bool SSIM>
__global__ __launch_bounds__(NT) void loss_backward_kernel(int C, int H, int W, const float* __restrict__ img, long long img_row,
							    long long img_ch, long long img_im, const float* __restrict__ gt,
							    long long gt_row, long long gt_ch, long long gt_im, LossTaps taps,
							    const float* __restrict__ dmaps, long long map_stride, float w_ssim, float w_l1,
							    float count, const float* __restrict__ grad_loss, int grad_per_image,
							    float* __restrict__ out_grad)
{
	__shared__ float s_in[SSIM ? 3 * HS * IN_LD : 1];
	__shared__ float s_h[SSIM ? 3 * HS * H_LD : 1];

	const int plane = blockIdx.z, b = plane / C, ch = plane - b * C;
	const int x0 = blockIdx.x * TS, y0 = blockIdx.y * TS;
	const float* px = img + (long long)b * img_im + (long long)ch * img_ch;
	const float* py = gt + (long long)b * gt_im + (long long)ch * gt_ch;
	const int c = threadIdx.x & 31, r0 = (threadIdx.x >> 5) * 4;
	const int gx = x0 + c;
	float f[3][4];
	if (SSIM) {
#pragma unroll
		for (int m = 0; m < 3; ++m)
			load_halo(s_in + m * HS * IN_LD, dmaps + m * map_stride + (long long)plane * H * W, W, H, W, y0, x0);
		__syncthreads();
		for (int i = threadIdx.x; i < HS * (TS / 4); i += NT) {
			const int r = i >> 3, c0 = (i & 7) * 4;
#pragma unroll
			for (int m = 0; m < 3; ++m) {
				float v[14], o[4];
#pragma unroll
				for (int k = 0; k < 14; ++k) v[k] = s_in[m * HS * IN_LD + r * IN_LD + c0 + k];
				taps4(v, taps, o);
#pragma unroll
				for (int j = 0; j < 4; ++j) s_h[m * HS * H_LD + r * H_LD + c0 + j] = o[j];
			}
		}
		__syncthreads();
#pragma unroll
		for (int m = 0; m < 3; ++m) vertical4(s_h + m * HS * H_LD, c, r0, taps, f[m]);
	}
	const float g = grad_loss[grad_per_image ? b : 0];
	const float ks = (g * w_ssim) / count, kl = (g * w_l1) / count;
#pragma unroll
	for (int j = 0; j < 4; ++j) {
		const int gy = y0 + r0 + j;
		if (gy >= H || gx >= W) continue;
		const float x = px[(long long)gy * img_row + gx], y = py[(long long)gy * gt_row + gx];
		const float d = x - y;
		float r = kl * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));   // sign(0) = 0 (torch's abs backward)
		if (SSIM) r += ks * (f[0][j] + 2.f * x * f[1][j] + y * f[2][j]);
		out_grad[(long long)plane * H * W + (long long)gy * W + gx] = r;
	}
}

// utils/loss_utils.py:26-28: exp(-(x - 5)^2 / 4.5) in double, stored as fp32, divided by their fp32 sum.  torch adds the 11
// floats in its vectorised order; the sum taken here is the correctly rounded one (added in double, then rounded), which is
// what that order yields -- adding them one after the other in fp32 lands one ulp lower and moves every tap.
// tests/test_loss.py holds the result against the window the reference built.
LossTaps make_taps()
{
	LossTaps t;
	float g[2 * RAD + 1];
	double sum = 0.0;
	for (int i = 0; i <= 2 * RAD; ++i) {
		const double d = (double)(i - RAD);
		g[i] = (float)exp(-(d * d) / 4.5);
		sum += (double)g[i];
	}
	const float fsum = (float)sum;
	for (int i = 0; i <= 2 * RAD; ++i) t.w[i] = g[i] / fsum;
	double m1 = 0.0, m2 = 0.0;
	for (int i = 0; i <= 2 * RAD; ++i) {
		m1 += (double)t.w[i];
		for (int j = 0; j <= 2 * RAD; ++j) m2 += (double)(float)(t.w[i] * t.w[j]);
	}
	t.mass = (float)(m2 / (m1 * m1) - 1.0);
	return t;
}

} // namespace

size_t photometric_loss_scratch_bytes(int B, int C, int H, int W)
{
	const size_t tiles = (size_t)((W + TS - 1) / TS) * (size_t)((H + TS - 1) / TS);
	return tiles * (size_t)B * (size_t)C * 2 * sizeof(double);
}

void photometric_loss_taps(float out[11])
{
	const LossTaps t = make_taps();
	for (int i = 0; i < 11; ++i) out[i] = t.w[i];
}

hipError_t launch_photometric_loss_forward(hipStream_t st, int B, int C, int H, int W, const float* img, const long long img_pitch[3],
					   const float* gt, const long long gt_pitch[3], float lambda, int mean_over_batch, float* out_loss,
					   float* out_ssim, float* out_l1, float* dmaps, void* scratch)
{
	const LossTaps taps = make_taps();
	const dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, B * C);
	const long long map_stride = (long long)B * C * H * W;
	double* partials = (double*)scratch;
	const bool with_ssim = out_ssim != nullptr;
#define SGS_LOSS_FWD(S, M)                                                                                                              \
	hipLaunchKernelGGL((loss_forward_kernel<S, M>), grid, dim3(NT), 0, st, C, H, W, img, img_pitch[0], img_pitch[1], img_pitch[2], gt, \
			   gt_pitch[0], gt_pitch[1], gt_pitch[2], taps, dmaps, map_stride, partials)
	if (!with_ssim) SGS_LOSS_FWD(false, false);
	else if (dmaps) SGS_LOSS_FWD(true, true);
	else SGS_LOSS_FWD(true, false);
#undef SGS_LOSS_FWD
	const long long tiles_per_plane = (long long)grid.x * grid.y;
	const int outs = mean_over_batch ? 1 : B;
	const long long tiles_per_out = tiles_per_plane * C * (mean_over_batch ? B : 1);
	const double count = (double)C * H * W * (mean_over_batch ? B : 1);
	hipLaunchKernelGGL(loss_finish_kernel, dim3(outs), dim3(NT), 0, st, partials, tiles_per_out, count, lambda, out_loss, out_ssim, out_l1);
	return hipGetLastError();
}

hipError_t launch_photometric_loss_backward(hipStream_t st, int B, int C, int H, int W, const float* img, const long long img_pitch[3],
					    const float* gt, const long long gt_pitch[3], float w_ssim, float w_l1, const float* dmaps,
					    const float* grad_loss, int mean_over_batch, float* out_grad)
{
	const LossTaps taps = make_taps();
	const dim3 grid((W + TS - 1) / TS, (H + TS - 1) / TS, B * C);
	const long long map_stride = (long long)B * C * H * W;
	const float count = (float)((double)C * H * W * (mean_over_batch ? B : 1));
#define SGS_LOSS_BWD(S)                                                                                                                  \
	hipLaunchKernelGGL((loss_backward_kernel<S>), grid, dim3(NT), 0, st, C, H, W, img, img_pitch[0], img_pitch[1], img_pitch[2], gt,    \
			   gt_pitch[0], gt_pitch[1], gt_pitch[2], taps, dmaps, map_stride, w_ssim, w_l1, count, grad_loss,                  \
			   mean_over_batch ? 0 : 1, out_grad)
	if (dmaps) SGS_LOSS_BWD(true);
	else SGS_LOSS_BWD(false);
#undef SGS_LOSS_BWD
	return hipGetLastError();
}

} // namespace sgs
