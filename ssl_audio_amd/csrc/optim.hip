// Multi-tensor LARS over a flat fp32 parameter buffer (utils/utils.py:150-189, the optimiser main.py:326-345 builds): every tensor of a
// train.FlatState in two launches, with no atomics and no host round trip.
//
// The tensors are segments of the flat buffer, described by a device table of int64 rows {start, count, chunk_base, flags}.  Each
// segment is cut into LARS_CHUNK-element chunks numbered from chunk_base; chunk c owns slot c of the partials workspace.
//   pass 1: per chunk, |p|^2 and |g + wd p|^2 summed in a fixed order inside the block -> partials[2c], partials[2c + 1];
//   pass 2: per segment, the block adds the segment's chunk partials in a fixed order (q = eta |p| / |dp|, 1 when a norm is 0 or the
//           segment is not adapted), then mu = momentum mu + q dp, p -= lr mu, and writes the bf16 mirror of p.
// Every block that works on a segment computes the same q from the same partials in the same order, so the step is bitwise
// reproducible.  lr comes per segment from a device row (FlatState.hyper), so a captured launch replays with the current value.
#include "common.h"
#include "../../include/ssl_audio_hip.h"

namespace {

constexpr int LARS_THREADS = 256;
constexpr int LARS_VEC = 8;                                        // elements per thread and pass: two float4 of p / g / mu, one bf16x8
constexpr int64_t LARS_CHUNK = 8192;                               // = SA_LARS_CHUNK in the header
static_assert(LARS_CHUNK % (LARS_THREADS * LARS_VEC) == 0, "a chunk is whole block passes");
constexpr int LARS_MAX_GRID = 2048;                                // cdna_hip_programming.md guideline 11: ~256 CUs x 8, the rest grid-strided

struct Seg {
  int64_t start, count, chunk_base, nchunks;
  int row;
  bool decay, adapt, valid;
};

__device__ __forceinline__ Seg load_seg(const int64_t* __restrict__ table, int s, int64_t n_total, int64_t n_chunks, int hyper_rows) {
  Seg r;
  r.start = table[4 * s + 0];
  r.count = table[4 * s + 1];
  r.chunk_base = table[4 * s + 2];
  const int64_t flags = table[4 * s + 3];
  r.row = (int)(flags & 0xff);
  r.decay = (flags >> 8) & 1;
  r.adapt = (flags >> 9) & 1;
  r.nchunks = (r.count + LARS_CHUNK - 1) / LARS_CHUNK;
  // a row that would reach outside the buffers, the workspace or the hyper rows is not touched (the host builds the table; this only
  // keeps a malformed one from writing out of bounds)
  r.valid = r.start >= 0 && (r.start % LARS_VEC) == 0 && r.count >= 0 && r.start + r.count <= n_total && r.chunk_base >= 0 &&
            r.chunk_base + r.nchunks <= n_chunks && r.row < hyper_rows;
  return r;
}

// the segment that holds chunk c: the last row whose chunk_base <= c (chunk_base ascends with the row index)
__device__ __forceinline__ int find_seg(const int64_t* __restrict__ table, int n_seg, int64_t c) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[4 * mid + 2] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// contiguous chunk range of this block: consecutive chunks mostly share a segment, so pass 2 reduces a segment's partials once per block
__device__ __forceinline__ void block_chunks(int64_t n_chunks, int64_t& c0, int64_t& c1) {
  const int64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
  c0 = (int64_t)blockIdx.x * per;
  c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
}

__global__ __launch_bounds__(LARS_THREADS) void lars_flat_norms_kernel(const float* __restrict__ p, const float* __restrict__ g, int64_t n_total,
                                                                       const int64_t* __restrict__ table, int n_seg, int64_t n_chunks,
                                                                       int hyper_rows, float wd, float* __restrict__ partials,
                                                                       const int32_t* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ float red[8];
  int64_t c0, c1;
  block_chunks(n_chunks, c0, c1);
  if (c0 >= c1) return;
  int s = find_seg(table, n_seg, c0);
  Seg sg = load_seg(table, s, n_total, n_chunks, hyper_rows);
  for (int64_t c = c0; c < c1; ++c) {
    while (s + 1 < n_seg && table[4 * (s + 1) + 2] <= c) sg = load_seg(table, ++s, n_total, n_chunks, hyper_rows);
    if (!sg.valid || !sg.adapt || c >= sg.chunk_base + sg.nchunks) continue;         // (block-uniform)
    const float wds = sg.decay ? wd : 0.f;
    const int64_t lo = (c - sg.chunk_base) * LARS_CHUNK;
    const int64_t len = (sg.count - lo < LARS_CHUNK ? sg.count - lo : LARS_CHUNK);
    const float* pc = p + sg.start + lo;
    const float* gc = g + sg.start + lo;
    float sp = 0.f, su = 0.f;
    for (int64_t j = (int64_t)threadIdx.x * LARS_VEC; j < len; j += LARS_THREADS * LARS_VEC) {
      if (j + LARS_VEC <= len) {
        const float4 p0 = *(const float4*)(pc + j), p1 = *(const float4*)(pc + j + 4);
        const float4 g0 = *(const float4*)(gc + j), g1 = *(const float4*)(gc + j + 4);
        const float pp[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = gg[k] + wds * pp[k];
          sp += pp[k] * pp[k];
          su += d * d;
        }
      } else {
        for (int64_t k = j; k < len; ++k) {
          const float d = gc[k] + wds * pc[k];
          sp += pc[k] * pc[k];
          su += d * d;
        }
      }
    }
    sp = block_sum_256(sp, red);
    su = block_sum_256(su, red + 4);
    if (threadIdx.x == 0) {
      partials[2 * c] = sp;
      partials[2 * c + 1] = su;
    }
  }
}

__global__ __launch_bounds__(LARS_THREADS) void lars_flat_update_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ mu,
                                                                        bf16_t* __restrict__ p_bf16, int64_t n_total, const int64_t* __restrict__ table,
                                                                        int n_seg, int64_t n_chunks, const float* __restrict__ hyper, int hyper_rows,
                                                                        int hyper_stride, float wd, float momentum, float eta,
                                                                        const float* __restrict__ partials, const int32_t* __restrict__ skip) {
  if (skip && *skip) return;
  __shared__ float red[8];
  int64_t c0, c1;
  block_chunks(n_chunks, c0, c1);
  if (c0 >= c1) return;
  int s = find_seg(table, n_seg, c0);
  Seg sg = load_seg(table, s, n_total, n_chunks, hyper_rows);
  int have = -1;                                                   // the segment q and lr below belong to
  float q = 1.f, lr = 0.f, wds = 0.f;
  for (int64_t c = c0; c < c1; ++c) {
    while (s + 1 < n_seg && table[4 * (s + 1) + 2] <= c) sg = load_seg(table, ++s, n_total, n_chunks, hyper_rows);
    if (!sg.valid || c >= sg.chunk_base + sg.nchunks) continue;        // (block-uniform)
    if (have != s) {
      have = s;
      lr = hyper[sg.row * hyper_stride];
      wds = sg.decay ? wd : 0.f;
      q = 1.f;
      if (sg.adapt) {
        float sp = 0.f, su = 0.f;
        for (int64_t k = threadIdx.x; k < sg.nchunks; k += LARS_THREADS) {
          sp += partials[2 * (sg.chunk_base + k)];
          su += partials[2 * (sg.chunk_base + k) + 1];
        }
        sp = block_sum_256(sp, red);
        su = block_sum_256(su, red + 4);
        const float pn = sqrtf(sp), un = sqrtf(su);
        q = (pn > 0.f && un > 0.f) ? eta * pn / un : 1.f;
      }
    }
    const int64_t lo = (c - sg.chunk_base) * LARS_CHUNK;
    const int64_t len = (sg.count - lo < LARS_CHUNK ? sg.count - lo : LARS_CHUNK);
    float* pc = p + sg.start + lo;
    const float* gc = g + sg.start + lo;
    float* mc = mu + sg.start + lo;
    bf16_t* bc = p_bf16 ? p_bf16 + sg.start + lo : nullptr;
    for (int64_t j = (int64_t)threadIdx.x * LARS_VEC; j < len; j += LARS_THREADS * LARS_VEC) {
      if (j + LARS_VEC <= len) {
        const float4 p0 = *(const float4*)(pc + j), p1 = *(const float4*)(pc + j + 4);
        const float4 g0 = *(const float4*)(gc + j), g1 = *(const float4*)(gc + j + 4);
        const float4 m0 = *(const float4*)(mc + j), m1 = *(const float4*)(mc + j + 4);
        float pp[8] = {p0.x, p0.y, p0.z, p0.w, p1.x, p1.y, p1.z, p1.w};
        const float gg[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w};
        float mm[8] = {m0.x, m0.y, m0.z, m0.w, m1.x, m1.y, m1.z, m1.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float d = (gg[k] + wds * pp[k]) * q;
          mm[k] = mm[k] * momentum + d;
          pp[k] = pp[k] - lr * mm[k];
        }
        *(float4*)(pc + j) = make_float4(pp[0], pp[1], pp[2], pp[3]);
        *(float4*)(pc + j + 4) = make_float4(pp[4], pp[5], pp[6], pp[7]);
        *(float4*)(mc + j) = make_float4(mm[0], mm[1], mm[2], mm[3]);
        *(float4*)(mc + j + 4) = make_float4(mm[4], mm[5], mm[6], mm[7]);
        if (bc)
          *(bf16x8*)(bc + j) = bf16x8{f2bf(pp[0]), f2bf(pp[1]), f2bf(pp[2]), f2bf(pp[3]), f2bf(pp[4]), f2bf(pp[5]), f2bf(pp[6]), f2bf(pp[7])};
      } else {
        for (int64_t k = j; k < len; ++k) {
          const float pk = pc[k];
          const float d = (gc[k] + wds * pk) * q;
          const float m = mc[k] * momentum + d;
          const float po = pk - lr * m;
          mc[k] = m;
          pc[k] = po;
          if (bc) bc[k] = f2bf(po);
        }
      }
    }
  }
}

inline int lars_grid(int64_t n_chunks) { return (int)(n_chunks < LARS_MAX_GRID ? n_chunks : LARS_MAX_GRID); }

}  // namespace

extern "C" int sa_lars_flat_step(float* p, const float* g, float* mu, void* p_bf16, int64_t n, const int64_t* segments, int32_t n_segments,
                                 int64_t n_chunks, const float* hyper, int32_t hyper_rows, int32_t hyper_stride, float weight_decay,
                                 float momentum, float eta, float* partials, const int32_t* skip_flag, void* stream) {
  SA_CHECK_ARG(p && g && mu && n >= 0 && n_segments >= 0 && n_chunks >= 0, "sa_lars_flat_step: bad args (p, g, mu, n >= 0, n_segments >= 0, n_chunks >= 0)");
  SA_CHECK_ARG(segments || n_segments == 0, "sa_lars_flat_step: segments is NULL");
  SA_CHECK_ARG(hyper && hyper_rows >= 1 && hyper_rows <= 256 && hyper_stride >= 1,
               "sa_lars_flat_step: hyper must hold 1..256 rows of stride >= 1 (lr of group r at hyper[r * hyper_stride])");
  SA_CHECK_ARG(partials || n_chunks == 0, "sa_lars_flat_step: partials is NULL (2 * n_chunks floats)");
  SA_CHECK_ARG(((((uintptr_t)p | (uintptr_t)g | (uintptr_t)mu | (uintptr_t)p_bf16) & 15) == 0),
               "sa_lars_flat_step: p, g, mu and p_bf16 must be 16-byte aligned");
  if (n_segments == 0 || n_chunks == 0 || n == 0) return 0;
  const int grid = lars_grid(n_chunks);
  hipLaunchKernelGGL(lars_flat_norms_kernel, dim3(grid), dim3(LARS_THREADS), 0, (hipStream_t)stream, p, g, n, segments, n_segments, n_chunks,
                     hyper_rows, weight_decay, partials, skip_flag);
  hipLaunchKernelGGL(lars_flat_update_kernel, dim3(grid), dim3(LARS_THREADS), 0, (hipStream_t)stream, p, g, mu, (bf16_t*)p_bf16, n, segments,
                     n_segments, n_chunks, hyper, hyper_rows, hyper_stride, weight_decay, momentum, eta, partials, skip_flag);
  SA_LAUNCH_CHECK("sa_lars_flat_step");
  return 0;
}
