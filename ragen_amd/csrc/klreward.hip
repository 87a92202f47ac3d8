// klreward.hip — the two steps around compute_advantage in the trainer's adv block (gfx950).
//
//  rmi_kl_reward              verl apply_kl_penalty / core_algos.kl_penalty (agent_trainer.py:613-615):
//                             token_level_rewards = token_level_scores - beta * kld, and the per-row
//                             sums current_kl is made of
//  rmi_rows_mean              the batch mean of per-row values (current_kl), one fixed order per n
//  rmi_length_weight_rows     the row lengths of grpo_advantage_length_weight (agent_trainer.py:637-639)
//  rmi_length_weight_finalize ... and the relative lengths (count + 1e-6) / mean(count)
//  rmi_row_div                advantages / relative_lengths.unsqueeze(-1) (agent_trainer.py:640), in place
// (rmi_grpo_outcome_scaled, the fused form of the last step, shares grpo_kernel in advantage.hip.)
//
// Exactness: every f32 operation is the reference's, in its order (the build compiles with
// -ffp-contract=off): d = old - ref, the estimator, kld * (float)(mask != 0) as a multiply (a
// non-finite log-prob under a zero mask gives NaN as torch does), (float)beta * kld rounded, then
// the subtract.  Row sums are fp64 over the f32 kld values in an order fixed by the COLUMN alone
// (below), so a row gives the same bits whatever its position in the batch, the shard it is in
// or the alignment of the tensors.
//
// Memory: a wave per row, kBlock / 64 rows per block.  A row is cut at the 16-byte boundaries
// of the flat index into 4-element groups: full groups move as 16-B accesses (and one dword of
// mask), the partial group at either end goes one element per lane; without 16-B aligned bases
// every group is moved element by element.  17 B per token, as rmi_gae.
#include <math.h>

#include "common.hpp"

namespace rmi {
namespace {

typedef float f4v __attribute__((ext_vector_type(4)));
constexpr double kStreamBytes = 256.0 * 1024 * 1024;  // a launch's traffic from which NT is used (as advantage.hip)
enum { kScalar = 0, kVec = 1, kVecNT = 2 };

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}
__device__ __forceinline__ long long wave_sum(long long x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  return x;
}

__device__ __forceinline__ uint32_t nz8(uint32_t x) {  // 0x01 per nonzero byte
  x |= x >> 4;
  x |= x >> 2;
  x |= x >> 1;
  return x & 0x01010101u;
}

// A row [o, e) of the flat index as 4-element groups: a head of h < 4 elements, nb full groups
// from b0 (a multiple of 4 when vec), a tail of nt < 4 elements.  Without vec the groups start
// at the row's first element (h = 0).
struct RowSpan {
  int64_t o, b0, nb;
  int h, nt;
};
__device__ __forceinline__ RowSpan row_span(int64_t row, int64_t L, bool vec) {
  const int64_t o = row * L, e = o + L;
  int64_t b0 = vec ? (o + 3) & ~(int64_t)3 : o;
  if (b0 > e) b0 = e;
  return RowSpan{o, b0, (e - b0) >> 2, (int)(b0 - o), (int)((e - b0) & 3)};
}

// core_algos.kl_penalty: 0 kl, 1 abs, 2 mse, 3 low_var_kl (clamp keeps a NaN, as torch.clamp)
template <int KIND>
__device__ __forceinline__ float kl_term(float old_lp, float ref_lp) {
  if (KIND == 3) {
    const float k = ref_lp - old_lp;
    const float x = (expf(k) - k) - 1.0f;
    return x < -10.0f ? -10.0f : (x > 10.0f ? 10.0f : x);
  }
  const float d = old_lp - ref_lp;
  if (KIND == 1) return fabsf(d);
  if (KIND == 2) return 0.5f * (d * d);
  return d;
}
template <int KIND>
__device__ __forceinline__ float kl_elem(float s, float old_lp, float ref_lp, bool in, float beta, float& reward) {
  const float kld = kl_term<KIND>(old_lp, ref_lp) * (float)in;
  reward = s - beta * kld;
  return kld;
}

// The row sum's order.  Column c belongs to class c % 256; a class is summed in column order,
// then lane m adds its classes (4m + 0, 1) + (4m + 2, 3) and the wave's xor butterfly adds the
// lanes.  Group j of the span (columns h + 4j ..) is worked on by lane j % 64, whose element e
// is of class (h + 4 * (j % 64) + e) % 256 for every j: the lane keeps one accumulator per e.
// The head is group -1 (lane 63, before its other groups), the tail group nb.  At the end the
// classes 4m .. 4m + 3 are fetched to lane m: element (f - h) & 3 of lane m, or of lane m - 1
// for f < h.
__device__ __forceinline__ double row_sum_classes(const double (&acc)[4], int h, int lane) {
  double v[4];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    const int e = (f - h) & 3;  // wave-uniform
    const double a = e == 0 ? acc[0] : (e == 1 ? acc[1] : (e == 2 ? acc[2] : acc[3]));
    v[f] = __shfl(a, f >= h ? lane : (lane + 63) & 63, 64);
  }
  return wave_sum((v[0] + v[1]) + (v[2] + v[3]));
}

template <int KIND, int MODE>
__global__ __launch_bounds__(kBlock) void kl_reward_kernel(const float* __restrict__ scores,
                                                           const float* __restrict__ old_lp,
                                                           const float* __restrict__ ref_lp,
                                                           const uint8_t* __restrict__ mask, int64_t B, int64_t L,
                                                           float beta, float* __restrict__ rewards,
                                                           double* __restrict__ row_stats) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= B) return;
  const RowSpan sp = row_span(row, L, MODE != kScalar);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  int cnt = 0;
  // head: element c on lane c, summed on lane 63 as element 4 - h + c of group -1
  if (sp.h) {
    float kld = 0.0f;
    if (lane < sp.h) {
      const int64_t i = sp.o + lane;
      const bool in = mask[i] != 0;
      float rw;
      kld = kl_elem<KIND>(scores[i], old_lp[i], ref_lp[i], in, beta, rw);
      rewards[i] = rw;
      cnt += in;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double x = (double)__shfl(kld, c, 64);
      const int e = 4 - sp.h + c;
#pragma unroll
      for (int k = 1; k < 4; ++k) acc[k] += (lane == 63 && c < sp.h && e == k) ? x : 0.0;
    }
  }
  // full groups
#pragma unroll 2
  for (int64_t j = lane; j < sp.nb; j += 64) {
    const int64_t i = sp.b0 + 4 * j;
    float s[4], po[4], pr[4], rw[4];
    uint32_t m4;
    if (MODE != kScalar) {
      // a streamed launch's loads are nontemporal too, as the GAE kernels' (8192 x 4096: 108-110 ->
      // 95-99 us, profiles/kl_reward/ab_nt_loads.txt); in-cache launches keep the cached form
      constexpr bool ntl = MODE == kVecNT;
      const f4v* ps = reinterpret_cast<const f4v*>(scores + i);
      const f4v* po4 = reinterpret_cast<const f4v*>(old_lp + i);
      const f4v* pr4 = reinterpret_cast<const f4v*>(ref_lp + i);
      const f4v a = ntl ? __builtin_nontemporal_load(ps) : *ps;
      const f4v b = ntl ? __builtin_nontemporal_load(po4) : *po4;
      const f4v c = ntl ? __builtin_nontemporal_load(pr4) : *pr4;
      m4 = nz8(*reinterpret_cast<const uint32_t*>(mask + i));
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[e] = a[e];
        po[e] = b[e];
        pr[e] = c[e];
      }
    } else {
      m4 = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[e] = scores[i + e];
        po[e] = old_lp[i + e];
        pr[e] = ref_lp[i + e];
        m4 |= (uint32_t)(mask[i + e] != 0) << (8 * e);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
      acc[e] += (double)kl_elem<KIND>(s[e], po[e], pr[e], (m4 >> (8 * e)) & 1u, beta, rw[e]);
    cnt += __popc(m4);
    if (MODE != kScalar) {
      const f4v y = {rw[0], rw[1], rw[2], rw[3]};
      if (MODE == kVecNT)
        __builtin_nontemporal_store(y, reinterpret_cast<f4v*>(rewards + i));
      else
        *reinterpret_cast<f4v*>(rewards + i) = y;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) rewards[i + e] = rw[e];
    }
  }
  // tail: element t on lane t, summed on lane nb % 64 as element t of group nb
  if (sp.nt) {
    float kld = 0.0f;
    if (lane < sp.nt) {
      const int64_t i = sp.b0 + 4 * sp.nb + lane;
      const bool in = mask[i] != 0;
      float rw;
      kld = kl_elem<KIND>(scores[i], old_lp[i], ref_lp[i], in, beta, rw);
      rewards[i] = rw;
      cnt += in;
    }
    const int owner = (int)(sp.nb & 63);
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const double x = (double)__shfl(kld, t, 64);
      acc[t] += (lane == owner && t < sp.nt) ? x : 0.0;
    }
  }
  const double sum = row_sum_classes(acc, sp.h, lane);
  const int n = wave_sum(cnt);
  if (lane == 0) {
    row_stats[2 * row + 0] = sum;
    row_stats[2 * row + 1] = (double)n;
  }
}

// out = mean_i x[i * stride] (/ den[i * stride] with den): thread t adds i = t, t + 1024, ..
// in order, the butterfly adds a wave's lanes, thread 0 the 16 waves in order.
__global__ __launch_bounds__(1024) void rows_mean_kernel(const double* __restrict__ x, const double* __restrict__ den,
                                                         int64_t n, int64_t stride, double* __restrict__ out) {
  __shared__ double red[16];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) s += den ? x[i * stride] / den[i * stride] : x[i * stride];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w];
    *out = t / (double)n;
  }
}

__global__ __launch_bounds__(kBlock) void length_rows_kernel(const uint8_t* __restrict__ mask, int64_t B, int64_t L,
                                                             int32_t* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= B) return;
  const uint8_t* p = mask + row * L;
  int64_t h = (int64_t)((4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3);  // bytes up to the first whole dword
  if (h > L) h = L;
  const int64_t nb = (L - h) >> 2;
  int c = 0;
  if (lane < h) c += p[lane] != 0;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p + h);
  for (int64_t k = lane; k < nb; k += 64) c += __popc(nz8(w[k]));
  const int64_t t = h + 4 * nb + lane;
  if (t < L) c += p[t] != 0;
  c = wave_sum(c);
  if (lane == 0) count[row] = c;
}

// rel = (count + 1e-6) / mean(count): the f32 add of torch's `sum + 1e-6` (16 -> 16.000001907,
// 32 -> 32.0) and the mean as the exact integer total rounded once over (float)n.
__global__ __launch_bounds__(1024) void length_finalize_kernel(const int32_t* __restrict__ count, int64_t n,
                                                               float* __restrict__ rel) {
  __shared__ long long red[16];
  long long s = 0;
  for (int64_t i = threadIdx.x; i < n; i += 1024) s += count[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  long long total = 0;
  for (int w = 0; w < 16; ++w) total += red[w];
  const float mean = __fdiv_rn((float)total, (float)n);
  for (int64_t i = threadIdx.x; i < n; i += 1024) rel[i] = __fdiv_rn(__fadd_rn((float)count[i], 1e-6f), mean);
}

template <bool VEC>
__global__ __launch_bounds__(kBlock) void row_div_kernel(float* __restrict__ x, const float* __restrict__ scale,
                                                         int64_t B, int64_t L) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (row >= B) return;
  const RowSpan sp = row_span(row, L, VEC);
  const float d = scale[row];
  if (lane < sp.h) x[sp.o + lane] = __fdiv_rn(x[sp.o + lane], d);
  for (int64_t j = lane; j < sp.nb; j += 64) {
    const int64_t i = sp.b0 + 4 * j;
    if (VEC) {
      f4v a = *reinterpret_cast<const f4v*>(x + i);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = __fdiv_rn(a[e], d);
      *reinterpret_cast<f4v*>(x + i) = a;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) x[i + e] = __fdiv_rn(x[i + e], d);
    }
  }
  const int64_t t = sp.b0 + 4 * sp.nb + lane;
  if (lane < sp.nt) x[t] = __fdiv_rn(x[t], d);
}

constexpr int64_t kMaxRows = 0x7FFFFFFFll * (kBlock / 64);  // a wave per row in a 1-D grid
inline dim3 row_grid(int64_t B) { return dim3((unsigned)((B + kBlock / 64 - 1) / (kBlock / 64))); }

template <int KIND>
void launch_kl_reward(int mode, hipStream_t s, const float* scores, const float* old_lp, const float* ref_lp,
                      const uint8_t* mask, int64_t B, int64_t L, float beta, float* rewards, double* row_stats) {
  if (mode == kVecNT)
    hipLaunchKernelGGL((kl_reward_kernel<KIND, kVecNT>), row_grid(B), dim3(kBlock), 0, s, scores, old_lp, ref_lp, mask,
                       B, L, beta, rewards, row_stats);
  else if (mode == kVec)
    hipLaunchKernelGGL((kl_reward_kernel<KIND, kVec>), row_grid(B), dim3(kBlock), 0, s, scores, old_lp, ref_lp, mask, B,
                       L, beta, rewards, row_stats);
  else
    hipLaunchKernelGGL((kl_reward_kernel<KIND, kScalar>), row_grid(B), dim3(kBlock), 0, s, scores, old_lp, ref_lp, mask,
                       B, L, beta, rewards, row_stats);
}

}  // namespace
}  // namespace rmi

RMI_API int rmi_kl_reward(const float* scores, const float* old_log_probs, const float* ref_log_prob,
                          const uint8_t* mask, int64_t B, int64_t L, double beta, int32_t kind, float* rewards,
                          double* row_stats, rmi_stream_t stream) {
  using namespace rmi;
  if (!scores || !old_log_probs || !ref_log_prob || !mask || !rewards || !row_stats || B < 0 || L < 0 || kind < 0 ||
      kind > 3)
    return RMI_EINVAL;
  if (B > kMaxRows) return RMI_EUNSUP;
  if (B == 0 || L == 0) return RMI_OK;
  const uintptr_t f32s = reinterpret_cast<uintptr_t>(scores) | reinterpret_cast<uintptr_t>(old_log_probs) |
                         reinterpret_cast<uintptr_t>(ref_log_prob) | reinterpret_cast<uintptr_t>(rewards);
  const bool vec = (f32s & 15) == 0 && (reinterpret_cast<uintptr_t>(mask) & 3) == 0;
  const bool nt = (double)B * (double)L * 17.0 > kStreamBytes;  // three f32 and the mask in, rewards out
  const int mode = vec ? (nt ? kVecNT : kVec) : kScalar;
  hipStream_t s = as_stream(stream);
  const float b = (float)beta;
  switch (kind) {
    case 0: launch_kl_reward<0>(mode, s, scores, old_log_probs, ref_log_prob, mask, B, L, b, rewards, row_stats); break;
    case 1: launch_kl_reward<1>(mode, s, scores, old_log_probs, ref_log_prob, mask, B, L, b, rewards, row_stats); break;
    case 2: launch_kl_reward<2>(mode, s, scores, old_log_probs, ref_log_prob, mask, B, L, b, rewards, row_stats); break;
    default: launch_kl_reward<3>(mode, s, scores, old_log_probs, ref_log_prob, mask, B, L, b, rewards, row_stats);
  }
  return launch_status();
}

RMI_API int rmi_rows_mean(const double* x, const double* den, int64_t n, int64_t stride, double* out,
                          rmi_stream_t stream) {
  using namespace rmi;
  if (!x || !out || n < 0 || stride < 1) return RMI_EINVAL;
  if (n == 0) return RMI_OK;
  hipLaunchKernelGGL(rows_mean_kernel, dim3(1), dim3(1024), 0, as_stream(stream), x, den, n, stride, out);
  return launch_status();
}

RMI_API int rmi_length_weight_finalize(const int32_t* count, int64_t n, float* rel, rmi_stream_t stream) {
  using namespace rmi;
  if (!count || !rel || n < 0) return RMI_EINVAL;
  if (n == 0) return RMI_OK;
  hipLaunchKernelGGL(length_finalize_kernel, dim3(1), dim3(1024), 0, as_stream(stream), count, n, rel);
  return launch_status();
}

RMI_API int rmi_length_weight_rows(const uint8_t* mask, int64_t B, int64_t L, int32_t* count, float* rel,
                                   rmi_stream_t stream) {
  using namespace rmi;
  if (B < 0 || L < 0 || (B > 0 && (!count || (L > 0 && !mask)))) return RMI_EINVAL;
  if (B > kMaxRows) return RMI_EUNSUP;
  if (B == 0) return RMI_OK;
  hipLaunchKernelGGL(length_rows_kernel, row_grid(B), dim3(kBlock), 0, as_stream(stream), mask, B, L, count);
  if (rel) hipLaunchKernelGGL(length_finalize_kernel, dim3(1), dim3(1024), 0, as_stream(stream), count, B, rel);
  return launch_status();
}

RMI_API int rmi_row_div(float* x, const float* scale, int64_t B, int64_t L, rmi_stream_t stream) {
  using namespace rmi;
  if (!x || !scale || B < 0 || L < 0) return RMI_EINVAL;
  if (B > kMaxRows) return RMI_EUNSUP;
  if (B == 0 || L == 0) return RMI_OK;
  if ((reinterpret_cast<uintptr_t>(x) & 15) == 0)
    hipLaunchKernelGGL(row_div_kernel<true>, row_grid(B), dim3(kBlock), 0, as_stream(stream), x, scale, B, L);
  else
    hipLaunchKernelGGL(row_div_kernel<false>, row_grid(B), dim3(kBlock), 0, as_stream(stream), x, scale, B, L);
  return launch_status();
}
