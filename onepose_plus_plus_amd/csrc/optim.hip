// Parameter update of the training step: global-norm gradient clipping + Adam / AdamW over a LIST of tensors in two launches.
//
// Reference: src/models/OnePosePlus/optimizers/optimizers.py:4-13 (torch.optim.Adam / AdamW) under Lightning's
// `gradient_clip_val: 0.5` (train.yaml:32, i.e. torch.nn.utils.clip_grad_norm_ before every update).  torch runs that as seven
// multi-tensor kernels of 14-28 launches each plus a foreach norm / stack / norm / clamp / foreach mul for the clip; here
//   grad_sqnorm_kernel   reads g once: one double partial (sum of squares x grad_scale^2) per workgroup, into a slot it owns
//   adam_step_kernel     every workgroup sums those partials in index order (same bits in every workgroup), forms the clip
//                        coefficient, then reads p, g, m, v and writes p, m, v of its chunk
// No atomics, no dependence on the order in which workgroups run: the same inputs give the same bits.
//
// Both kernels walk two device tables the host builds once (opp_optim_plan): one opp_optim_tensor per tensor, one
// opp_optim_chunk per workgroup.  A chunk is at most OPP_OPTIM_CHUNK elements of ONE tensor, so the tensor's pointers and its
// alignment are wave-uniform: float4 accesses when all four pointers are 16-byte aligned (chunk starts are multiples of 4
// elements, so the tensor's base pointers decide), else a 4-byte path; the last n % 4 elements of a tensor take a scalar tail.
// HBM-bound: 4 bytes x (1 + 4 + 3) per element.
#include <math.h>

#include "../../include/opp_hip.h"
#include "opp_internal.h"

namespace {

constexpr int kThreads = 256;
constexpr int kChunk = OPP_OPTIM_CHUNK;
constexpr int kVec = kChunk / 4 / kThreads;      // float4 per lane and array in a full chunk
static_assert(kChunk % (4 * kThreads) == 0 && kVec % 4 == 0, "a full chunk is whole batches of 4 float4 per lane");

// sum over the workgroup in a fixed order (lanes by shuffle, then the four waves through LDS); every lane returns the total
__device__ inline double block_sum(double x, double* lds) {
  for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();                               // lds may still be read from a previous call
  if ((threadIdx.x & 63) == 0) lds[wave] = x;
  __syncthreads();
  double total = lds[0];
  for (int w = 1; w < kThreads / 64; ++w) total += lds[w];
  return total;
}

__global__ __launch_bounds__(kThreads) void grad_sqnorm_kernel(const opp_optim_tensor* __restrict__ tensors,
                                                               const opp_optim_chunk* __restrict__ chunks, double scale_sq,
                                                               double* __restrict__ partials) {
  __shared__ double lds[kThreads / 64];
  const opp_optim_chunk ck = chunks[blockIdx.x];
  const float* __restrict__ g = tensors[ck.tensor].g + ck.start;
  const int len = ck.len;
  double acc = 0.0;
  if ((reinterpret_cast<uintptr_t>(g) & 15) == 0) {
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    const int n4 = len >> 2;
    if (n4 == kChunk / 4) {                      // full chunk: every load of the lane in flight at once
      float4 x[kVec];
#pragma unroll
      for (int j = 0; j < kVec; ++j) x[j] = g4[threadIdx.x + j * kThreads];
#pragma unroll
      for (int j = 0; j < kVec; ++j)
        acc += (double)x[j].x * x[j].x + (double)x[j].y * x[j].y + (double)x[j].z * x[j].z + (double)x[j].w * x[j].w;
    } else {
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        const float4 x = g4[i];
        acc += (double)x.x * x.x + (double)x.y * x.y + (double)x.z * x.z + (double)x.w * x.w;
      }
    }
    for (int i = (n4 << 2) + threadIdx.x; i < len; i += kThreads) acc += (double)g[i] * g[i];
  } else {
    for (int i = threadIdx.x; i < len; i += kThreads) acc += (double)g[i] * g[i];
  }
  const double total = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = total * scale_sq;
}

struct AdamArgs {
  float max_norm;          // clipping threshold (used when n_partials > 0)
  float grad_scale;
  float decay_mul;         // AdamW: 1 - lr * wd (1 when off)
  float decay_add;         // Adam: wd (0 when off)
  float w1;                // 1 - beta1
  float beta2, w2;         // beta2, 1 - beta2
  float bc2_sqrt;          // sqrt(1 - beta2^t)
  float eps;
  float neg_step;          // -lr / (1 - beta1^t)
  int decoupled_decay, coupled_decay;
};

// one element in torch's order of operations (torch/optim/adam.py `_single_tensor_adam`; lerp as ATen's: two forms around w = 0.5)
__device__ inline void adam_one(float& p, float g, float& m, float& v, float coef, const AdamArgs& a) {
  g = g * a.grad_scale * coef;
  if (a.decoupled_decay) p *= a.decay_mul;
  if (a.coupled_decay) g += a.decay_add * p;
  const float d = g - m;
  m = a.w1 < 0.5f ? m + a.w1 * d : g - d * (1.f - a.w1);
  v = v * a.beta2 + a.w2 * g * g;
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
  p += a.neg_step * (m / denom);
}

__device__ inline void adam_four(float4& p, const float4& g, float4& m, float4& v, float coef, const AdamArgs& a) {
  adam_one(p.x, g.x, m.x, v.x, coef, a);
  adam_one(p.y, g.y, m.y, v.y, coef, a);
  adam_one(p.z, g.z, m.z, v.z, coef, a);
  adam_one(p.w, g.w, m.w, v.w, coef, a);
}

__global__ __launch_bounds__(kThreads) void adam_step_kernel(const opp_optim_tensor* __restrict__ tensors,
                                                             const opp_optim_chunk* __restrict__ chunks,
                                                             const double* __restrict__ partials, int n_partials,
                                                             float* __restrict__ norm_out, AdamArgs a) {
  __shared__ double lds[kThreads / 64];
  float coef = 1.f;
  if (n_partials > 0) {                          // clipping: the global norm, summed in the same order by every workgroup
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += kThreads) acc += partials[i];
    const float total_norm = (float)sqrt(block_sum(acc, lds));
    const float c = a.max_norm / (total_norm + 1e-6f);
    coef = c > 1.f ? 1.f : c;                    // a NaN norm propagates, as through torch's clamp
    if (blockIdx.x == 0 && threadIdx.x == 0 && norm_out) *norm_out = total_norm;
  }
  const opp_optim_chunk ck = chunks[blockIdx.x];
  const opp_optim_tensor t = tensors[ck.tensor];
  float* __restrict__ p = t.p + ck.start;
  const float* __restrict__ g = t.g + ck.start;
  float* __restrict__ m = t.m + ck.start;
  float* __restrict__ v = t.v + ck.start;
  const int len = ck.len;
  const uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                         reinterpret_cast<uintptr_t>(v);
  if ((bits & 15) == 0) {
    float4* __restrict__ p4 = reinterpret_cast<float4*>(p);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(m);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(v);
    const int n4 = len >> 2;
    if (n4 == kChunk / 4) {                      // full chunk: batches of 4 float4 per array, 16 independent loads in flight per lane
#pragma unroll 1
      for (int b = 0; b < kVec; b += 4) {
        float4 xp[4], xg[4], xm[4], xv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = threadIdx.x + (b + j) * kThreads;
          xp[j] = p4[i];
          xg[j] = g4[i];
          xm[j] = m4[i];
          xv[j] = v4[i];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = threadIdx.x + (b + j) * kThreads;
          adam_four(xp[j], xg[j], xm[j], xv[j], coef, a);
          p4[i] = xp[j];
          m4[i] = xm[j];
          v4[i] = xv[j];
        }
      }
    } else {
      for (int i = threadIdx.x; i < n4; i += kThreads) {
        float4 xp = p4[i], xm = m4[i], xv = v4[i];
        const float4 xg = g4[i];
        adam_four(xp, xg, xm, xv, coef, a);
        p4[i] = xp;
        m4[i] = xm;
        v4[i] = xv;
      }
    }
    for (int i = (n4 << 2) + threadIdx.x; i < len; i += kThreads) adam_one(p[i], g[i], m[i], v[i], coef, a);
  } else {
    for (int i = threadIdx.x; i < len; i += kThreads) adam_one(p[i], g[i], m[i], v[i], coef, a);
  }
}

}  // namespace

extern "C" int opp_optim_chunk_elems(void) { return kChunk; }

extern "C" int opp_optim_plan(const long long* numel, int n_tensors, opp_optim_chunk* chunks, long long max_chunks,
                              long long* n_chunks) {
  OPP_CHECK_ARG(n_tensors >= 0 && (numel || n_tensors == 0) && n_chunks, "optim_plan: bad argument");
  long long count = 0;
  for (int t = 0; t < n_tensors; ++t) {
    OPP_CHECK_ARG(numel[t] >= 0, "optim_plan: tensor %d has a negative element count", t);
    count += (numel[t] + kChunk - 1) / kChunk;
  }
  OPP_CHECK_ARG(count <= 0x7fffffffLL, "optim_plan: %lld chunks do not fit one grid", count);
  *n_chunks = count;
  if (!chunks) return OPP_OK;                    // size query
  OPP_CHECK_ARG(max_chunks >= count, "optim_plan: the chunk table holds %lld entries, %lld needed", max_chunks, count);
  long long c = 0;
  for (int t = 0; t < n_tensors; ++t)
    for (long long start = 0; start < numel[t]; start += kChunk, ++c) {
      const long long left = numel[t] - start;
      chunks[c].tensor = t;
      chunks[c].len = (int)(left < kChunk ? left : kChunk);
      chunks[c].start = start;
    }
  return OPP_OK;
}

extern "C" int opp_grad_sqnorm(const opp_optim_tensor* tensors, const opp_optim_chunk* chunks, int n_chunks, double grad_scale,
                               double* partials, void* stream) {
  OPP_CHECK_ARG(n_chunks >= 0, "grad_sqnorm: bad argument");
  if (n_chunks == 0) return OPP_OK;
  OPP_CHECK_ARG(tensors && chunks && partials, "grad_sqnorm: bad argument");
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3(n_chunks), dim3(kThreads), 0, (hipStream_t)stream, tensors, chunks,
                     grad_scale * grad_scale, partials);
  OPP_CHECK_LAUNCH("grad_sqnorm_kernel");
  return OPP_OK;
}

extern "C" int opp_adam_step(const opp_optim_tensor* tensors, const opp_optim_chunk* chunks, int n_chunks, const double* partials,
                             int n_partials, double max_norm, float* norm_out, double grad_scale, double lr, double beta1,
                             double beta2, double eps, double weight_decay, int decoupled, double bc1, double bc2, void* stream) {
  OPP_CHECK_ARG(n_chunks >= 0 && n_partials >= 0, "adam_step: bad argument");
  OPP_CHECK_ARG(n_partials == 0 || partials, "adam_step: clipping needs the partial sums of opp_grad_sqnorm");
  OPP_CHECK_ARG(bc1 > 0.0 && bc2 > 0.0, "adam_step: bias corrections must be positive (1 - beta^t with t >= 1)");
  if (n_chunks == 0) return OPP_OK;
  OPP_CHECK_ARG(tensors && chunks, "adam_step: bad argument");
  AdamArgs a;
  a.max_norm = (float)max_norm;
  a.grad_scale = (float)grad_scale;
  a.decoupled_decay = weight_decay != 0.0 && decoupled;
  a.coupled_decay = weight_decay != 0.0 && !decoupled;
  a.decay_mul = (float)(1.0 - lr * weight_decay);
  a.decay_add = (float)weight_decay;
  a.w1 = (float)(1.0 - beta1);
  a.beta2 = (float)beta2;
  a.w2 = (float)(1.0 - beta2);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.eps = (float)eps;
  a.neg_step = (float)(-(lr / bc1));
  hipLaunchKernelGGL(adam_step_kernel, dim3(n_chunks), dim3(kThreads), 0, (hipStream_t)stream, tensors, chunks, partials, n_partials,
                     norm_out, a);
  OPP_CHECK_LAUNCH("adam_step_kernel");
  return OPP_OK;
}
