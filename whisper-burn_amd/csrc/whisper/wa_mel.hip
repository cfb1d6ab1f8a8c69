// wa_mel.hip -- log-mel front-end kernels.
//
// Reference: src/audio/mel.rs:126-228 (compute_log / stft) driven by
// src/transcribe.rs:44-76.  Two launches per batch of clips:
//
//   mel_power_kernel  one workgroup per 8 frames of one clip: reflect-padded,
//                     windowed frames -> 201-bin DFT (f64 accumulation over
//                     the symmetric half, so the spectrum is the exact DFT of
//                     the f32 windowed frame rounded once to f32, i.e. at
//                     least as accurate as the reference's f32 rustfft) ->
//                     |X|^2 (f32) -> mel filterbank (f32, the reference's
//                     product/sum order) -> log10(max(v, 1e-10)), written
//                     transposed [clip][mel][frame], plus the workgroup max.
//   mel_norm_kernel   clip max = max of the 375 workgroup maxima; clamp to
//                     max - 8 and (v + 4) / 4, in place (mel.rs:136-154).
//
// Windows of long recordings (wa_long_mel_max / wa_long_mel_windows) run the
// same frame body, mel_frames, on the zero-extended signal:
//
//   mel_stream_max_kernel  once per recording: every raw frame, maxima only
//                          (flat workgroup list over ragged recordings), then
//                          mel_stream_reduce_kernel, one workgroup each.
//   mel_window_kernel      the 3000 frames from `seek` of each clip's
//                          recording, normalised in the same pass against the
//                          recording's maximum, zeros past the content.
//
// Cost per 30 s clip: 3000 frames x 201 bins x 398 f64 FMA (the symmetric
// DFT) = 0.24 G FMA + 3000 x ~2 x 201 filterbank MACs; HBM traffic is 1.9 MB
// in + 2 x 1.5 MB out -- a compute-bound, sub-millisecond step next to the
// encoder.
#include <hip/hip_runtime.h>

#include <cmath>

#include "wa_mel.hpp"

namespace wa {
namespace {

constexpr int kThreads = 256;
constexpr int kHalf = kMelNfft / 2;  // 200
constexpr int kFr = kMelFramesPerWg;

// Sample p of the reflect-padded 480 400-sample signal (mel.rs:179-193) of a
// clip already padded / truncated to 480 000 samples (transcribe.rs:45-52):
// padded[p] = s[200 - p] on the left, s[p - 200] inside, s[479998 - i] at
// i = p - 480 200 on the right.  Samples at or past n are the zero padding.
__device__ __forceinline__ float padded_sample(const float* __restrict__ a, int64_t n, int p) {
  int s;
  if (p < kHalf)
    s = kHalf - p;
  else if (p < kMelChunk + kHalf)
    s = p - kHalf;
  else
    s = (kMelChunk - 2) - (p - (kMelChunk + kHalf));
  return (int64_t)s < n ? a[s] : 0.0f;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// LDS of one workgroup's frames: 38.6 KB.
struct MelLds {
  double sx[kFr][kHalf + 1];
  double dx[kFr][kHalf];
  double tw[2 * kMelNfft];
  float pw[kFr][kMelBins + 3];
  float red[kThreads / 64];
};

// The frame body every mel kernel shares: nfr <= 8 frames whose first sample
// is fetch(p0), frame fr starting kMelHop * fr further on.  fetch(p) is sample
// p (int64) of the kernel's padded signal; store(m, fr, v) takes raw[m][fr] =
// log10(max(mel power, 1e-10)).  Returns the maximum of the stored values,
// valid in thread 0.  A frame's value depends on its 400 samples only.
template <class Fetch, class Store>
__device__ __forceinline__ float mel_frames(MelLds& L, Fetch fetch, int64_t p0, int nfr, int n_mels,
                                            const float* __restrict__ window, const float* __restrict__ filters,
                                            const int* __restrict__ range, const double* __restrict__ twiddle,
                                            Store store) {
  // s_j = x_j + x_{400-j}, d_j = x_j - x_{400-j} (exact in f64); s_0 = x_0,
  // s_200 = x_200.  Re X_k = s_0 + (-1)^k s_200 + sum_j s_j cos(2 pi jk/400),
  // Im X_k = -sum_j d_j sin(2 pi jk/400), j = 1..199.
  const int tid = threadIdx.x;
  for (int i = tid; i < 2 * kMelNfft; i += kThreads) L.tw[i] = twiddle[i];
  for (int i = tid; i < kFr * (kHalf + 1); i += kThreads) {
    const int fr = i / (kHalf + 1), j = i - fr * (kHalf + 1);
    double s = 0.0, d = 0.0;
    if (fr < nfr) {
      const int64_t p = p0 + (int64_t)fr * kMelHop;
      // windowed sample, one f32 multiply as mel.rs:208
      const float xj = __fmul_rn(fetch(p + j), window[j]);
      if (j == 0 || j == kHalf) {
        s = xj;
      } else {
        const float xm = __fmul_rn(fetch(p + kMelNfft - j), window[kMelNfft - j]);
        s = (double)xj + (double)xm;
        d = (double)xj - (double)xm;
      }
    }
    L.sx[fr][j] = s;
    if (j < kHalf) L.dx[fr][j] = d;
  }
  __syncthreads();

  const int k = tid;
  if (k < kMelBins) {
    double re[kFr], im[kFr];
    const double sgn = (k & 1) ? -1.0 : 1.0;
#pragma unroll
    for (int fr = 0; fr < kFr; ++fr) {
      re[fr] = L.sx[fr][0] + sgn * L.sx[fr][kHalf];
      im[fr] = 0.0;
    }
    int idx = k;  // (j * k) mod 400 at j = 1
    for (int j = 1; j < kHalf; ++j) {
      const double c = L.tw[idx], s = L.tw[kMelNfft + idx];
#pragma unroll
      for (int fr = 0; fr < kFr; ++fr) {
        re[fr] = fma(L.sx[fr][j], c, re[fr]);
        im[fr] = fma(L.dx[fr][j], s, im[fr]);
      }
      idx += k;
      if (idx >= kMelNfft) idx -= kMelNfft;
    }
#pragma unroll
    for (int fr = 0; fr < kFr; ++fr) {
      const float r = (float)re[fr], i = (float)im[fr];
      L.pw[fr][k] = __fadd_rn(__fmul_rn(r, r), __fmul_rn(i, i));  // norm_sqr, mel.rs:111
    }
  }
  __syncthreads();

  // filterbank: lanes 8 apart in idx share a mel, consecutive lanes write
  // consecutive frames of the transposed output
  float mx = -INFINITY;
  for (int i = tid; i < n_mels * kFr; i += kThreads) {
    const int m = i / kFr, fr = i - m * kFr;
    if (fr >= nfr) continue;
    const int lo = range[2 * m], hi = range[2 * m + 1];
    const float* f = filters + (int64_t)m * kMelBins;
    float acc = 0.0f;  // mel.rs:237, zero taps contribute exact zeros and are skipped
    for (int kk = lo; kk <= hi; ++kk) acc = __fadd_rn(acc, __fmul_rn(f[kk], L.pw[fr][kk]));
    // mel.rs:132; f64 log10 rounded once to f32 = the correctly rounded
    // log10f of the reference's libm (device log10f is 1 ulp off at 1e-10)
    const float v = (float)log10((double)fmaxf(acc, 1e-10f));
    store(m, fr, v);
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) L.red[tid >> 6] = mx;
  __syncthreads();
  float r = L.red[0];
  for (int w = 1; w < kThreads / 64; ++w) r = fmaxf(r, L.red[w]);
  return r;
}

__global__ __launch_bounds__(kThreads) void mel_power_kernel(const float* __restrict__ audio, int64_t n,
                                                             int64_t ld, int n_mels,
                                                             const float* __restrict__ window,
                                                             const float* __restrict__ filters,
                                                             const int* __restrict__ range,
                                                             const double* __restrict__ twiddle,
                                                             float* __restrict__ part, float* __restrict__ out) {
  __shared__ MelLds L;
  const int b = blockIdx.y;
  const int f0 = blockIdx.x * kFr;
  const int nfr = min(kFr, kMelFrames - f0);
  const float* a = audio + (int64_t)b * ld;
  float* o = out + (int64_t)b * n_mels * kMelFrames + f0;
  const float r = mel_frames(
      L, [&](int64_t p) { return padded_sample(a, n, (int)p); }, (int64_t)f0 * kMelHop, nfr, n_mels, window, filters,
      range, twiddle, [&](int m, int fr, float v) { o[(int64_t)m * kMelFrames + fr] = v; });
  if (threadIdx.x == 0) part[(int64_t)b * kMelWgPerClip + blockIdx.x] = r;
}

// ---- windows of long recordings (wa_long_mel_max / wa_long_mel_windows) ----
// The extended signal of a recording of n samples: zeros past its end, the
// 200 samples before its start reflected about sample 0 (no right reflection:
// the signal is zero-extended).  p is the index into the signal padded by 200
// on the left, so frame f starts at p = 160 f.
__device__ __forceinline__ float extended_sample(const float* __restrict__ a, int64_t n, int64_t p) {
  int64_t s = p - kHalf;
  if (s < 0) s = -s;
  return s < n ? a[s] : 0.0f;
}

// One workgroup per 8 raw frames of one recording, over the flat list of all
// recordings' workgroups: wg_first[r] .. wg_first[r + 1] - 1 are recording r's
// (host-built prefix table).  Keeps the workgroup's maximum only.
__global__ __launch_bounds__(kThreads) void mel_stream_max_kernel(const float* __restrict__ audio,
                                                                  const MelStream* __restrict__ streams,
                                                                  int n_streams, int n_mels,
                                                                  const float* __restrict__ window,
                                                                  const float* __restrict__ filters,
                                                                  const int* __restrict__ range,
                                                                  const double* __restrict__ twiddle,
                                                                  float* __restrict__ part) {
  __shared__ MelLds L;
  const int64_t wg = blockIdx.x;
  int lo = 0, hi = n_streams - 1;  // the last recording whose first workgroup is <= wg
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (streams[mid].wg_first <= wg) lo = mid; else hi = mid - 1;
  }
  const MelStream s = streams[lo];
  const int64_t f0 = (wg - s.wg_first) * kFr;
  const int64_t left = s.frames - f0;  // >= 1: the table holds no empty workgroup
  const int nfr = left < kFr ? (int)left : kFr;
  const float* a = audio + s.offset;
  const int64_t n = s.n;
  const float r = mel_frames(
      L, [&](int64_t p) { return extended_sample(a, n, p); }, f0 * kMelHop, nfr, n_mels, window, filters, range,
      twiddle, [](int, int, float) {});
  if (threadIdx.x == 0) part[wg] = r;
}

// Recording r's maximum: its workgroups' maxima and the -10 of every frame past them.
__global__ __launch_bounds__(kThreads) void mel_stream_reduce_kernel(const float* __restrict__ part,
                                                                     const MelStream* __restrict__ streams,
                                                                     float* __restrict__ max_out) {
  __shared__ float red[kThreads / 64];
  const MelStream s = streams[blockIdx.x];
  const int64_t w0 = s.wg_first, w1 = w0 + (s.frames + kFr - 1) / kFr;
  float m = -10.0f;
  for (int64_t i = w0 + threadIdx.x; i < w1; i += kThreads) m = fmaxf(m, part[i]);
  m = wave_max(m);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kThreads / 64; ++w) m = fmaxf(m, red[w]);
    max_out[blockIdx.x] = m;
  }
}

// One workgroup per 8 frames of one window: frames seek + j, j < size =
// min(3000, n / 160 - seek), normalised against the recording's maximum in the
// same pass; exact zeros from `size` on.
__global__ __launch_bounds__(kThreads) void mel_window_kernel(const float* __restrict__ audio,
                                                              const MelWindow* __restrict__ wins,
                                                              const float* __restrict__ max_dev, int n_mels,
                                                              const float* __restrict__ window,
                                                              const float* __restrict__ filters,
                                                              const int* __restrict__ range,
                                                              const double* __restrict__ twiddle,
                                                              float* __restrict__ out) {
  __shared__ MelLds L;
  const MelWindow w = wins[blockIdx.y];
  const int f0 = blockIdx.x * kFr;  // 375 * 8 = 3000: every workgroup has 8 columns
  const int64_t content = w.n / kMelHop - w.seek;
  const int size = content < kMelFrames ? (int)(content > 0 ? content : 0) : kMelFrames;
  const int nfr = min(kFr, size - f0);  // <= 0: the zero tail only
  float* o = out + (int64_t)blockIdx.y * n_mels * kMelFrames + f0;
  if (nfr < kFr)
    for (int i = threadIdx.x; i < n_mels * kFr; i += kThreads) {
      const int m = i / kFr, fr = i - m * kFr;
      if (fr >= nfr) o[(int64_t)m * kMelFrames + fr] = 0.0f;
    }
  if (nfr <= 0) return;
  const float lo = max_dev[w.max_index] - 8.0f;
  const float* a = audio + w.offset;
  const int64_t n = w.n;
  mel_frames(
      L, [&](int64_t p) { return extended_sample(a, n, p); }, ((int64_t)w.seek + f0) * kMelHop, nfr, n_mels, window,
      filters, range, twiddle,
      [&](int m, int fr, float v) { o[(int64_t)m * kMelFrames + fr] = (fmaxf(v, lo) + 4.0f) / 4.0f; });
}

__global__ __launch_bounds__(kThreads) void mel_norm_kernel(const float* __restrict__ part, int per_clip,
                                                            float* __restrict__ out) {
  __shared__ float smx;
  const int b = blockIdx.y;
  if (threadIdx.x < 64) {
    float m = -INFINITY;
    for (int i = threadIdx.x; i < kMelWgPerClip; i += 64) m = fmaxf(m, part[(int64_t)b * kMelWgPerClip + i]);
    m = wave_max(m);
    if (threadIdx.x == 0) smx = m;
  }
  __syncthreads();
  const float lo = smx - 8.0f;  // mel.rs:141
  const int i4 = blockIdx.x * kThreads + threadIdx.x;
  if (i4 * 4 >= per_clip) return;
  float4* p = reinterpret_cast<float4*>(out + (int64_t)b * per_clip) + i4;
  float4 v = *p;
  v.x = (fmaxf(v.x, lo) + 4.0f) / 4.0f;  // mel.rs:145, 152
  v.y = (fmaxf(v.y, lo) + 4.0f) / 4.0f;
  v.z = (fmaxf(v.z, lo) + 4.0f) / 4.0f;
  v.w = (fmaxf(v.w, lo) + 4.0f) / 4.0f;
  *p = v;
}

size_t align16(size_t x) { return (x + 15) & ~size_t(15); }

// The sections of the packed device constants (mel_pack_consts).
struct MelConsts {
  const float* window;
  const float* filters;
  const int* range;
  const double* twiddle;
};
MelConsts unpack_consts(const uint8_t* consts, int n_mels) {
  MelConsts c;
  c.window = reinterpret_cast<const float*>(consts);
  size_t off = align16(kMelNfft * 4);
  c.filters = reinterpret_cast<const float*>(consts + off);
  off += align16((size_t)n_mels * kMelBins * 4);
  c.range = reinterpret_cast<const int*>(consts + off);
  off += align16((size_t)n_mels * 8);
  c.twiddle = reinterpret_cast<const double*>(consts + off);
  return c;
}
}  // namespace

hipError_t launch_log_mel(const float* audio, int B, int64_t n_samples, int64_t ld_audio, int n_mels,
                          const uint8_t* consts, float* part, float* out, hipStream_t st) {
  const MelConsts c = unpack_consts(consts, n_mels);
  const int64_t n = n_samples < kMelChunk ? n_samples : kMelChunk;
  hipLaunchKernelGGL(mel_power_kernel, dim3(kMelWgPerClip, B), dim3(kThreads), 0, st, audio, n, ld_audio, n_mels,
                     c.window, c.filters, c.range, c.twiddle, part, out);
  const int per_clip = n_mels * kMelFrames;
  const int g = (per_clip / 4 + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(mel_norm_kernel, dim3(g, B), dim3(kThreads), 0, st, part, per_clip, out);
  return hipGetLastError();
}

hipError_t launch_long_mel_max(const float* audio, const MelStream* streams, int n_streams, int64_t n_wg, int n_mels,
                               const uint8_t* consts, float* part, float* max_out, hipStream_t st) {
  const MelConsts c = unpack_consts(consts, n_mels);
  hipLaunchKernelGGL(mel_stream_max_kernel, dim3((unsigned)n_wg), dim3(kThreads), 0, st, audio, streams, n_streams,
                     n_mels, c.window, c.filters, c.range, c.twiddle, part);
  hipLaunchKernelGGL(mel_stream_reduce_kernel, dim3(n_streams), dim3(kThreads), 0, st, part, streams, max_out);
  return hipGetLastError();
}

hipError_t launch_long_mel_windows(const float* audio, const MelWindow* wins, int B, const float* max_dev, int n_mels,
                                   const uint8_t* consts, float* out, hipStream_t st) {
  const MelConsts c = unpack_consts(consts, n_mels);
  hipLaunchKernelGGL(mel_window_kernel, dim3(kMelWgPerClip, B), dim3(kThreads), 0, st, audio, wins, max_dev, n_mels,
                     c.window, c.filters, c.range, c.twiddle, out);
  return hipGetLastError();
}

}  // namespace wa
