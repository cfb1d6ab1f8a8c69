// wa_mel.cpp -- the log-mel front-end entries (wa_log_mel, wa_long_mel_max,
// wa_long_mel_windows, wa_mel_filterbank) and their per-device state.
// Kernels: wa_mel.hip.
#include <map>
#include <mutex>

#include "wa_mel.hpp"
#include "wa_model.hpp"

using namespace wa;

// Per-device constants (window, filterbank, twiddles; per n_mels) and the
// per-workgroup-max scratch, allocated on first use outside stream capture.
namespace {
struct MelDevice {
  std::map<int, uint8_t*> consts;
  float* part = nullptr;
  int part_clips = 0;
  // windows of long recordings: the recordings' table and per-workgroup maxima
  // of wa_long_mel_max, the clips' descriptors of wa_long_mel_windows; the
  // tables are staged in pinned memory and uploaded on the launch stream
  // (*_uploaded: the table's last upload, awaited before its staging is rewritten)
  MelStream* streams = nullptr;
  MelStream* streams_host = nullptr;
  int streams_cap = 0;
  float* long_part = nullptr;
  int64_t long_part_cap = 0;
  MelWindow* wins = nullptr;
  MelWindow* wins_host = nullptr;
  int wins_cap = 0;
  hipEvent_t streams_uploaded = nullptr, wins_uploaded = nullptr;
};
std::mutex g_mel_mu;
std::map<int, MelDevice> g_mel;

wq4_status not_capturing(hipStream_t st, const char* who) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  WA_HIP(hipStreamIsCapturing(st, &cs));
  if (cs != hipStreamCaptureStatusNone)
    return fail(WQ4_EINVAL, std::string(who) + ": run once outside stream capture first (allocates)");
  return WQ4_OK;
}

// The (device, n_mels) constants, created on first use.
wq4_status mel_consts(MelDevice& md, int n_mels, hipStream_t st, const char* who, uint8_t** out) {
  uint8_t*& c = md.consts[n_mels];
  if (!c) {
    WA_TRY(not_capturing(st, who));
    const MelBank bank = make_mel_bank(n_mels);
    std::vector<uint8_t> host(mel_const_bytes(n_mels));
    mel_pack_consts(bank, host.data());
    WA_HIP(hipMalloc(reinterpret_cast<void**>(&c), host.size()));
    WA_HIP(hipMemcpy(c, host.data(), host.size(), hipMemcpyHostToDevice));
  }
  *out = c;
  return WQ4_OK;
}

// A device array and its pinned staging of at least `need` entries.
template <class T>
wq4_status grow_table(T*& dev, T*& host, int& cap, int need, hipStream_t st, const char* who) {
  if (cap >= need) return WQ4_OK;
  WA_TRY(not_capturing(st, who));
  WA_HIP(hipDeviceSynchronize());
  if (dev) WA_HIP(hipFree(dev));
  if (host) WA_HIP(hipHostFree(host));
  dev = host = nullptr;
  cap = 0;
  WA_HIP(hipMalloc(reinterpret_cast<void**>(&dev), (size_t)need * sizeof(T)));
  WA_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), (size_t)need * sizeof(T), 0));
  cap = need;
  return WQ4_OK;
}

// The staging may be rewritten once the last upload from it has run.
wq4_status staging_free(hipEvent_t& uploaded) {
  if (!uploaded) WA_HIP(hipEventCreateWithFlags(&uploaded, hipEventDisableTiming));
  WA_HIP(hipEventSynchronize(uploaded));
  return WQ4_OK;
}
}  // namespace

extern "C" {

wq4_status wa_log_mel(int device, const float* audio_dev, int n_clips, int64_t n_samples, int64_t ld_audio,
                      int n_mels, float* mel_dev, void* stream) {
  if (!mel_dev || (!audio_dev && n_samples > 0)) return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1) return fail(WQ4_EINVAL, "n_clips must be >= 1");
  if (n_samples < 0 || ld_audio < n_samples) return fail(WQ4_EINVAL, "need 0 <= n_samples <= ld_audio");
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  WA_HIP(hipSetDevice(device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mel_mu);
  MelDevice& md = g_mel[device];
  uint8_t* c = nullptr;
  WA_TRY(mel_consts(md, n_mels, st, "wa_log_mel", &c));
  if (md.part_clips < n_clips) {
    WA_TRY(not_capturing(st, "wa_log_mel"));
    WA_HIP(hipDeviceSynchronize());
    if (md.part) WA_HIP(hipFree(md.part));
    md.part = nullptr;
    md.part_clips = 0;
    WA_HIP(hipMalloc(reinterpret_cast<void**>(&md.part), (size_t)n_clips * kMelWgPerClip * sizeof(float)));
    md.part_clips = n_clips;
  }
  WA_HIP(launch_log_mel(audio_dev, n_clips, n_samples, ld_audio, n_mels, c, md.part, mel_dev, st));
  return WQ4_OK;
}

wq4_status wa_long_mel_max(int device, const float* audio_dev, int n_streams, const int64_t* offset,
                           const int64_t* n_samples, int n_mels, float* max_dev, void* stream) {
  if (!audio_dev || !offset || !n_samples || !max_dev) return fail(WQ4_EINVAL, "null argument");
  if (n_streams < 1) return fail(WQ4_EINVAL, "n_streams must be >= 1");
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  int64_t n_wg = 0;
  for (int r = 0; r < n_streams; ++r) {
    if (offset[r] < 0 || n_samples[r] < 0 || n_samples[r] >= kMelLongMaxSamples)
      return fail(WQ4_EINVAL, "need offset >= 0 and 0 <= n_samples < 160 * (2^31 - 3001)");
    n_wg += (mel_stream_frames(n_samples[r]) + kMelFramesPerWg - 1) / kMelFramesPerWg;
  }
  if (n_wg > 2147483647LL) return fail(WQ4_EINVAL, "more than 2^31 - 1 workgroups of frames in one call");
  WA_HIP(hipSetDevice(device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mel_mu);
  MelDevice& md = g_mel[device];
  uint8_t* c = nullptr;
  WA_TRY(mel_consts(md, n_mels, st, "wa_long_mel_max", &c));
  WA_TRY(grow_table(md.streams, md.streams_host, md.streams_cap, n_streams, st, "wa_long_mel_max"));
  if (md.long_part_cap < n_wg) {
    WA_TRY(not_capturing(st, "wa_long_mel_max"));
    WA_HIP(hipDeviceSynchronize());
    if (md.long_part) WA_HIP(hipFree(md.long_part));
    md.long_part = nullptr;
    md.long_part_cap = 0;
    WA_HIP(hipMalloc(reinterpret_cast<void**>(&md.long_part), (size_t)n_wg * sizeof(float)));
    md.long_part_cap = n_wg;
  }
  WA_TRY(staging_free(md.streams_uploaded));
  int64_t wg = 0;
  for (int r = 0; r < n_streams; ++r) {
    const int64_t frames = mel_stream_frames(n_samples[r]);
    md.streams_host[r] = MelStream{offset[r], n_samples[r], frames, wg};
    wg += (frames + kMelFramesPerWg - 1) / kMelFramesPerWg;
  }
  WA_HIP(hipMemcpyAsync(md.streams, md.streams_host, (size_t)n_streams * sizeof(MelStream), hipMemcpyHostToDevice, st));
  WA_HIP(hipEventRecord(md.streams_uploaded, st));
  WA_HIP(launch_long_mel_max(audio_dev, md.streams, n_streams, n_wg, n_mels, c, md.long_part, max_dev, st));
  return WQ4_OK;
}

wq4_status wa_long_mel_windows(int device, const float* audio_dev, int n_clips, const int64_t* offset,
                               const int64_t* n_samples, const int32_t* seek, const int32_t* max_index,
                               const float* max_dev, int n_mels, float* mel_dev, void* stream) {
  if (!audio_dev || !offset || !n_samples || !seek || !max_index || !max_dev || !mel_dev)
    return fail(WQ4_EINVAL, "null argument");
  if (n_clips < 1 || n_clips > 65535) return fail(WQ4_EINVAL, "n_clips must be in [1, 65535]");
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  for (int c = 0; c < n_clips; ++c) {
    if (offset[c] < 0 || n_samples[c] < 0 || n_samples[c] >= kMelLongMaxSamples)
      return fail(WQ4_EINVAL, "need offset >= 0 and 0 <= n_samples < 160 * (2^31 - 3001)");
    if (seek[c] < 0 || seek[c] >= n_samples[c] / kMelHop)
      return fail(WQ4_EINVAL, "need 0 <= seek < n_samples / 160");
    if (max_index[c] < 0) return fail(WQ4_EINVAL, "max_index must be >= 0");
  }
  WA_HIP(hipSetDevice(device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::lock_guard<std::mutex> lk(g_mel_mu);
  MelDevice& md = g_mel[device];
  uint8_t* c = nullptr;
  WA_TRY(mel_consts(md, n_mels, st, "wa_long_mel_windows", &c));
  WA_TRY(grow_table(md.wins, md.wins_host, md.wins_cap, n_clips, st, "wa_long_mel_windows"));
  WA_TRY(staging_free(md.wins_uploaded));
  for (int i = 0; i < n_clips; ++i) md.wins_host[i] = MelWindow{offset[i], n_samples[i], seek[i], max_index[i]};
  WA_HIP(hipMemcpyAsync(md.wins, md.wins_host, (size_t)n_clips * sizeof(MelWindow), hipMemcpyHostToDevice, st));
  WA_HIP(hipEventRecord(md.wins_uploaded, st));
  WA_HIP(launch_long_mel_windows(audio_dev, md.wins, n_clips, max_dev, n_mels, c, mel_dev, st));
  return WQ4_OK;
}

wq4_status wa_mel_filterbank(int n_mels, float* filters_out, float* window_out) {
  if (n_mels < 1 || n_mels > kMelMaxMels) return fail(WQ4_EINVAL, "n_mels must be in [1, 256]");
  const MelBank bank = make_mel_bank(n_mels);
  if (filters_out) std::memcpy(filters_out, bank.filters.data(), bank.filters.size() * sizeof(float));
  if (window_out) std::memcpy(window_out, bank.window.data(), bank.window.size() * sizeof(float));
  return WQ4_OK;
}

}  // extern "C"
