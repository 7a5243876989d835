// The rest of an optimisation step after loss.backward() (train.py:154-180): Adam over several tensors in ONE launch, with an optional
// per-row visibility mask, and the three densification statistics of add_densification_stats without a host read.
//
// adam_multi_kernel.  The host passes a table of tensor descriptors BY VALUE in the kernel arguments (no H2D copy, no sync) together
// with a prefix table of chunk counts: a chunk is ADAM_CHUNK = 1024 consecutive elements of one tensor, one 16-byte group per thread.
// The grid is capped (ADAM_GRID_CAP workgroups) and strides over the chunks of all tensors.  A tensor whose four pointers are all 16-byte
// aligned moves 16-byte groups and finishes its numel % 4 tail by element; any other tensor goes by element throughout.
//
// The arithmetic contract (every operation a separate correctly rounded float32 operation; the file is built with -ffp-contract=off,
// sqrtf and / are hipcc's correctly rounded defaults):
//     m' = (b1*m) + (c1*g)        v' = (b2*v) + (c2*(g*g))        den = (sqrtf(v') / r) + e        p' = p - (s * (m' / den))
//
// Mask: an element whose row (element index / width) is not visible is neither loaded nor stored.  The mask byte is tested BEFORE the
// loads, and the loads and stores sit under that test, so a wave whose lanes are all invisible branches round them (s_cbranch_execz)
// and issues nothing but its mask reads.  width % 4 == 0: a 16-byte group lies in one row, one mask byte decides it.  Otherwise a group
// can straddle two rows and is handled by element.
#include "sgs_kernels.h"

namespace sgs {

namespace {

constexpr int ADAM_NT = 256;
constexpr int ADAM_CHUNK = ADAM_NT * 4;   // elements per (workgroup, iteration)
constexpr int ADAM_GRID_CAP = 2048;       // 256 CUs x 8 workgroups of 4 waves: full occupancy, the rest is the stride loop

__device__ __forceinline__ void adam_element(float& p, const float g, float& m, float& v, const AdamTensor& t)
{
	const float m1 = (t.b1 * m) + (t.c1 * g);
	const float v1 = (t.b2 * v) + (t.c2 * (g * g));
	const float den = (sqrtf(v1) / t.r) + t.e;
	p = p - (t.s * (m1 / den));
	m = m1;
	v = v1;
}

__device__ __forceinline__ void adam_scalar_at(const AdamTensor& t, long long i)
{
	float p = t.param[i], m = t.exp_avg[i], v = t.exp_avg_sq[i];
	adam_element(p, t.grad[i], m, v, t);
	t.param[i] = p;
	t.exp_avg[i] = m;
	t.exp_avg_sq[i] = v;
}

typedef float v4f __attribute__((ext_vector_type(4)));

template <bool MASKED>
__global__ void __launch_bounds__(ADAM_NT) adam_multi_kernel(const AdamTable tab)
{
	for (int vb = blockIdx.x; vb < tab.chunk_start[tab.n]; vb += gridDim.x) {
		// (tensor, chunk) of this iteration: uniform over the workgroup, at most SGS_ADAM_MAX_TENSORS scalar compares
		int ti = 0;
		while (ti + 1 < tab.n && vb >= tab.chunk_start[ti + 1]) ++ti;
		const AdamTensor& t = tab.t[ti];
		const long long base = (long long)(vb - tab.chunk_start[ti]) * ADAM_CHUNK;   // first element of the chunk
		// row of an element of this chunk: one 64-bit division per chunk, 32-bit ones per element (width < 2^31 - ADAM_CHUNK, host-checked)
		long long row0 = 0;
		unsigned rem0 = 0;
		if (MASKED) {
			row0 = base / t.width;
			rem0 = (unsigned)(base - row0 * t.width);
		}
		if (t.vec4) {
			const long long i = base + 4 * (int)threadIdx.x;
			if (i + 4 <= t.numel) {
				bool whole = true, any = true;
				bool vis[4] = {true, true, true, true};
				if (MASKED) {
					if ((t.width & 3u) == 0) {
						whole = any = tab.visible[row0 + (rem0 + 4u * threadIdx.x) / t.width] != 0;
					} else {
#pragma unroll
						for (int k = 0; k < 4; ++k) vis[k] = tab.visible[row0 + (rem0 + 4u * threadIdx.x + k) / t.width] != 0;
						whole = vis[0] && vis[1] && vis[2] && vis[3];
						any = vis[0] || vis[1] || vis[2] || vis[3];
					}
				}
				if (whole) {
					v4f p = *reinterpret_cast<const v4f*>(t.param + i);
					// (the gradient is read once and never again: a nontemporal load, measured 2 % (1M x 512) to 6 % (six groups)
					// faster than a plain one; nontemporal forms of the other loads and of the stores measured no gain -- DESIGN.md 5.17)
					const v4f g = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(t.grad + i));
					v4f m = *reinterpret_cast<const v4f*>(t.exp_avg + i);
					v4f v = *reinterpret_cast<const v4f*>(t.exp_avg_sq + i);
#pragma unroll
					for (int k = 0; k < 4; ++k) {
						float pk = p[k], mk = m[k], vk = v[k];
						adam_element(pk, g[k], mk, vk, t);
						p[k] = pk;
						m[k] = mk;
						v[k] = vk;
					}
					*reinterpret_cast<v4f*>(t.param + i) = p;
					*reinterpret_cast<v4f*>(t.exp_avg + i) = m;
					*reinterpret_cast<v4f*>(t.exp_avg_sq + i) = v;
				} else if (any) {   // a group across a visible row and an invisible one
#pragma unroll
					for (int k = 0; k < 4; ++k)
						if (vis[k]) adam_scalar_at(t, i + k);
				}
			} else {   // the numel % 4 tail elements, in the tensor's last chunk only
				for (long long j = i; j < t.numel; ++j)
					if (!MASKED || tab.visible[row0 + (rem0 + (unsigned)(j - base)) / t.width] != 0) adam_scalar_at(t, j);
			}
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const unsigned off = k * ADAM_NT + threadIdx.x;   // consecutive lanes, consecutive elements
				const long long i = base + off;
				if (i < t.numel && (!MASKED || tab.visible[row0 + (rem0 + off) / t.width] != 0)) adam_scalar_at(t, i);
			}
		}
	}
}

// per Gaussian: train.py:158-161 + gaussian_model.py:608-612, the three statements that index with a boolean mask
__global__ void __launch_bounds__(256) densify_stats_kernel(int P, const float* __restrict__ viewspace_grad, long long grad_row_pitch,
							     const int* __restrict__ radii, const uint8_t* __restrict__ visible_in,
							     float* __restrict__ accum, float* __restrict__ denom, float* __restrict__ max_radii2D,
							     uint8_t* __restrict__ visible_out)
{
	for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += gridDim.x * blockDim.x) {
		const int rad = radii[i];
		const bool vis = visible_in ? visible_in[i] != 0 : rad > 0;
		if (visible_out) visible_out[i] = vis ? 1 : 0;
		if (!vis) continue;
		const float gx = viewspace_grad[(long long)i * grad_row_pitch], gy = viewspace_grad[(long long)i * grad_row_pitch + 1];
		accum[i] += sqrtf((gx * gx) + (gy * gy));
		denom[i] += 1.0f;
		max_radii2D[i] = fmaxf(max_radii2D[i], (float)rad);
	}
}

} // namespace

int adam_chunk_elements() { return ADAM_CHUNK; }

hipError_t launch_adam_multi(hipStream_t st, const AdamTable& tab)
{
	const int total = tab.chunk_start[tab.n];
	if (total <= 0) return hipSuccess;
	const int grid = total < ADAM_GRID_CAP ? total : ADAM_GRID_CAP;
	if (tab.visible)
		hipLaunchKernelGGL(adam_multi_kernel<true>, dim3(grid), dim3(ADAM_NT), 0, st, tab);
	else
		hipLaunchKernelGGL(adam_multi_kernel<false>, dim3(grid), dim3(ADAM_NT), 0, st, tab);
	return hipGetLastError();
}

hipError_t launch_densify_stats(hipStream_t st, int P, const float* viewspace_grad, long long grad_row_pitch, const int* radii,
				const uint8_t* visible_in, float* accum, float* denom, float* max_radii2D, uint8_t* visible_out)
{
	if (P <= 0) return hipSuccess;
	const int blocks = (P + 255) / 256;
	hipLaunchKernelGGL(densify_stats_kernel, dim3(blocks < 2048 ? blocks : 2048), dim3(256), 0, st, P, viewspace_grad, grad_row_pitch, radii,
			   visible_in, accum, denom, max_radii2D, visible_out);
	return hipGetLastError();
}

} // namespace sgs
