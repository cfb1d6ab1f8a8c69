// wa_weights.cpp -- where the model's weights come from (the synthetic
// generator or a GGUF file) and how they reach the device (loader.rs).
#include <atomic>
#include <cmath>
#include <thread>

#include "wa_model.hpp"

using namespace wa;

namespace {

// ----------------------------------------------- synthetic weights --
uint64_t fnv1a64(const char* s) {
  uint64_t h = 0xCBF29CE484222325ull;
  for (; *s; ++s) {
    h ^= (uint8_t)*s;
    h *= 0x100000001B3ull;
  }
  return h;
}

inline uint64_t splitmix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// fn(a, b) over [0, n) in chunks on up to 16 host threads (every element is
// computed from its index alone: the values do not depend on the split)
template <class F>
void parallel_for(int64_t n, F fn) {
  unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (n < (1 << 16)) nt = 1;
  std::vector<std::thread> th;
  const int64_t chunk = (n + nt - 1) / nt;
  for (unsigned t = 0; t < nt; ++t) {
    const int64_t a = t * chunk, b = std::min(n, a + chunk);
    if (a >= b) break;
    th.emplace_back([=] { fn(a, b); });
  }
  for (auto& x : th) x.join();
}

// oracle/oracle.py:synth_uniform -- bit-identical (compiled -ffp-contract=off).
void synth_uniform(uint64_t seed, const std::string& name, int64_t n, float lo, float hi, float* out) {
  const uint64_t key = seed ^ fnv1a64(name.c_str());
  const float span = (float)((double)hi - (double)lo);
  parallel_for(n, [&](int64_t a, int64_t b) {
    for (int64_t i = a; i < b; ++i) {
      const float u = (float)(splitmix64(key + (uint64_t)i) >> 40);
      const float unit = u * (float)(1.0 / 16777216.0);
      const float t = unit * span;
      out[i] = lo + t;
    }
  });
}

float lin_scale(int k) { return (float)(1.5 / std::sqrt((double)k)); }

// bytes of a [rows, k] linear weight in raw GGUF form (Source::linear)
size_t linear_bytes(int wtype, int64_t rows, int k) {
  return wtype == 1 ? (size_t)(rows * k) * 2 : (size_t)(rows * k / 32) * 18;
}

struct SynthSource : Source {
  uint64_t seed;
  explicit SynthSource(uint64_t s) : seed(s) {}
  bool f32(const std::string& name, int64_t n, float lo, float hi, bool optional, std::vector<float>& out) override {
    // Whisper's attention key projections have no bias (loader.rs:205-210)
    if (optional && name.size() > 9 && name.compare(name.size() - 9, 9, ".key.bias") == 0) return false;
    out.resize((size_t)n);
    synth_uniform(seed, name, n, lo, hi, out.data());
    return true;
  }
  bool linear(const std::string& name, int rows, int k, int wtype, uint8_t* dst) override {
    std::vector<float> w((size_t)rows * k);
    synth_uniform(seed, name, (int64_t)rows * k, -lin_scale(k), lin_scale(k), w.data());
    if (wtype == 1) {
      uint16_t* h = reinterpret_cast<uint16_t*>(dst);
      for (size_t i = 0; i < w.size(); ++i) h[i] = __builtin_bit_cast(uint16_t, (_Float16)w[i]);
      return true;
    }
    const int64_t nblk = (int64_t)rows * k / 32;
    parallel_for(nblk, [&](int64_t a, int64_t b) {
      (void)wq4_quantize_q4_0(w.data() + a * 32, (b - a) * 32, dst + a * 18);
    });
    return true;
  }
};

// f16 (IEEE binary16, little-endian) -> f32, exact (half 2.7.1 semantics).
float f16_to_f32(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }

struct GgufSource : Source {
  const GgufFile& g;
  explicit GgufSource(const GgufFile& f) : g(f) {}
  bool bad(const std::string& m) {
    err = m;
    return false;
  }
  // loader.rs:47-104 (F32 / F16 1-D and 2-D tensors, 3-D conv weights)
  bool f32(const std::string& name, int64_t n, float, float, bool optional, std::vector<float>& out) override {
    const GgufTensor* t = g.find(name);
    if (!t) return optional ? false : bad("Tensor '" + name + "' not found");
    if (t->type != kGgmlF32 && t->type != kGgmlF16) return bad("Expected F32/F16 for '" + name + "', got Q4_0");
    if ((int64_t)t->elements() != n)
      return bad("Tensor '" + name + "' has " + std::to_string(t->elements()) + " elements, expected " +
                 std::to_string(n));
    const uint8_t* p = g.data(*t);
    if (!p) return bad("Tensor '" + name + "' data lies outside the file");
    out.resize((size_t)n);
    if (t->type == kGgmlF32) {
      std::memcpy(out.data(), p, (size_t)n * 4);
    } else {
      for (int64_t i = 0; i < n; ++i) out[(size_t)i] = f16_to_f32((uint16_t)(p[2 * i] | (p[2 * i + 1] << 8)));
    }
    return true;
  }
  // loader.rs:106-144: Q4_0 only; GGUF dims are [in_features, out_features].
  // config 5: F16 linear weights (the reference loader rejects them)
  bool linear(const std::string& name, int rows, int k, int wtype, uint8_t* dst) override {
    const bool h = wtype == 1;
    const GgufTensor* t = g.find(name);
    if (!t) return bad("Tensor '" + name + "' not found");
    if (t->type != (h ? kGgmlF16 : kGgmlQ4_0)) {
      const std::string got = t->type == kGgmlF32 ? "F32" : h ? "Q4_0" : "F16";
      return bad(h ? "Expected F16 for weight '" + name + "' (an F16 checkpoint), got " + got
                   : "Expected Q4_0 for weight '" + name + "', got " + got + ". Use the conversion script.");
    }
    if (t->dims.size() != 2 || t->dims[0] != (uint64_t)k || t->dims[1] != (uint64_t)rows)
      return bad(std::string(h ? "F16" : "Q4") + " weight '" + name + "' has the wrong shape (expected [" +
                 std::to_string(rows) + ", " + std::to_string(k) + "])");
    const uint8_t* p = g.data(*t);
    if (!p) return bad("Tensor '" + name + "' data lies outside the file");
    std::memcpy(dst, p, t->nbytes());
    return true;
  }
};

struct Builder {
  wa_model* m;
  Source& src;
  wq4_status st = WQ4_OK;

  void* upload(const void* host, size_t n) {
    void* p = m->dev.alloc<uint8_t>(n);
    if (!p || hipMemcpy(p, host, n, hipMemcpyHostToDevice) != hipSuccess) {
      st = fail(WQ4_ENOMEM, "upload failed");
      return nullptr;
    }
    m->bytes += n;
    return p;
  }
  float* upload(const std::vector<float>& v) { return static_cast<float*>(upload(v.data(), v.size() * 4)); }
  std::vector<float> get(const std::string& name, int64_t n, float lo, float hi) {
    std::vector<float> v;
    if (st == WQ4_OK && !src.f32(name, n, lo, hi, false, v)) st = fail(WQ4_EINVAL, src.err);
    if (v.size() != (size_t)n) v.assign((size_t)n, 0.0f);
    return v;
  }
  float* vec(const std::string& name, int64_t n, float lo, float hi) { return upload(get(name, n, lo, hi)); }
  // host bytes of the GGUF linear weights `names` [n_i, k], row-concatenated;
  // returns their total rows (0: failed)
  int64_t gather(const std::vector<std::string>& names, const std::vector<int>& rows, int k, std::vector<uint8_t>& h) {
    if (st != WQ4_OK) return 0;
    int64_t total = 0;
    for (int r : rows) total += r;
    h.resize(linear_bytes(m->wtype, total, k));
    size_t off = 0;
    for (size_t i = 0; i < names.size(); ++i) {
      if (!src.linear(names[i], rows[i], k, m->wtype, h.data() + off)) {
        st = fail(WQ4_EINVAL, src.err);
        return 0;
      }
      off += linear_bytes(m->wtype, rows[i], k);
    }
    return total;
  }
  // Linear weights of several GGUF tensors [n_i, k], row-concatenated (a
  // fused projection): Q4_0 blocks, or f16 halves for an F16 model.
  // decode_step = false: the tensor never runs at <= 32 rows (encoder), so
  // the decode-step kernel's second weight copy is not built.
  wq4_tensor* q4(const std::vector<std::string>& names, const std::vector<int>& rows, int k, bool decode_step = true) {
    const unsigned cflags = decode_step ? 0u : WQ4_TENSOR_NO_DECODE_STEP;
    std::vector<uint8_t> h;
    const int64_t total = gather(names, rows, k, h);
    if (total == 0) return nullptr;
    const bool f16 = m->wtype == 1;
    wq4_tensor* t = nullptr;
    const wq4_status s =
        f16 ? wq4_tensor_create_f16_ex(m->device, reinterpret_cast<const uint16_t*>(h.data()), total, k, cflags, &t)
            : wq4_tensor_create_ex(m->device, h.data(), h.size(), total, k, cflags, &t);
    if (s != WQ4_OK) st = fail(s, std::string(f16 ? "F16 weight upload: " : "Q4 upload: ") + wq4_last_error());
    m->bytes += wq4_tensor_device_bytes(t);
    return t;
  }
  // One linear weight [rows, k] uploaded in its raw GGUF form (Q4_0 blocks,
  // or f16 halves for an F16 model) for kernels that dequantize it directly.
  uint8_t* raw(const std::string& name, int rows, int k) {
    std::vector<uint8_t> h;
    if (gather({name}, {rows}, k, h) == 0) return nullptr;
    return static_cast<uint8_t*>(upload(h.data(), h.size()));
  }
  // bias vector of a fused projection: absent biases (attention key) are 0.
  float* bias_cat(const std::vector<std::string>& names, int n) {
    std::vector<float> v;
    for (const auto& nm : names) {
      std::vector<float> b;
      if (st == WQ4_OK && src.f32(nm, n, -0.02f, 0.02f, true, b)) {
        v.insert(v.end(), b.begin(), b.end());
      } else {
        if (!src.err.empty()) st = fail(WQ4_EINVAL, src.err);
        v.insert(v.end(), n, 0.0f);
      }
    }
    return upload(v);
  }
  // conv weight [N, C, 3] (GGUF dims [3, C, N], loader.rs:254-268) ->
  // [N][kk*C + c] (im2col order, layers.rs:118-121)
  float* conv(const std::string& name, int N, int C) {
    auto w = get(name, (int64_t)N * C * 3, -lin_scale(3 * C), lin_scale(3 * C));
    return upload(conv_weight_im2col(w.data(), N, C));
  }
};

}  // namespace

namespace wa {

Config preset(int variant) {
  switch (variant) {
    case WA_LARGE_V3:  // config.rs:32-47; vocab = rows of the HF/GGUF embedding
      return {128, 1500, 1280, 20, 32, 448, 1280, 20, 32, 51866, 100};
    case WA_MEDIUM:  // config.rs:49-63
      return {80, 1500, 1024, 16, 24, 448, 1024, 16, 24, 51865, 99};
    default:  // parity-test configuration (not a released model)
      return {80, 1500, 384, 6, 2, 448, 384, 6, 2, 51866, 100};
  }
}

std::vector<float> conv_weight_im2col(const float* w, int N, int C) {
  std::vector<float> t((size_t)N * 3 * C);
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < C; ++c)
      for (int kk = 0; kk < 3; ++kk) t[(size_t)n * 3 * C + kk * C + c] = w[((size_t)n * C + c) * 3 + kk];
  return t;
}

std::unique_ptr<Source> synth_source(uint64_t seed) { return std::make_unique<SynthSource>(seed); }
std::unique_ptr<Source> gguf_source(const GgufFile& f) { return std::make_unique<GgufSource>(f); }

// Every weight of the model (loader.rs:279-377 load_encoder / load_decoder).
wq4_status build_model(wa_model* m, Source& src) {
  const Config& c = m->cfg;
  const int D = c.n_audio_state, F = 4 * D, Dt = c.n_text_state, Ft = 4 * Dt;
  Builder B{m, src};
  m->conv1_wt = B.conv("encoder.conv1.weight", D, c.n_mels);
  m->conv1_b = B.vec("encoder.conv1.bias", D, -0.02f, 0.02f);
  m->conv2_wt = B.conv("encoder.conv2.weight", D, D);
  m->conv2_b = B.vec("encoder.conv2.bias", D, -0.02f, 0.02f);
  m->enc_pos = B.vec("encoder.positional_embedding", (int64_t)c.n_audio_ctx * D, -0.1f, 0.1f);
  m->enc.resize(c.n_audio_layer);
  for (int i = 0; i < c.n_audio_layer; ++i) {
    const std::string p = "encoder.blocks." + std::to_string(i);
    EncLayer& L = m->enc[i];
    L.ln1_w = B.vec(p + ".attn_ln.weight", D, 0.9f, 1.1f);
    L.ln1_b = B.vec(p + ".attn_ln.bias", D, -0.05f, 0.05f);
    L.qkv = B.q4({p + ".attn.query.weight", p + ".attn.key.weight", p + ".attn.value.weight"}, {D, D, D}, D, false);
    L.qkv_b = B.bias_cat({p + ".attn.query.bias", p + ".attn.key.bias", p + ".attn.value.bias"}, D);
    L.out = B.q4({p + ".attn.out.weight"}, {D}, D, false);
    L.out_b = B.vec(p + ".attn.out.bias", D, -0.02f, 0.02f);
    L.ln2_w = B.vec(p + ".mlp_ln.weight", D, 0.9f, 1.1f);
    L.ln2_b = B.vec(p + ".mlp_ln.bias", D, -0.05f, 0.05f);
    L.fc1 = B.q4({p + ".mlp.0.weight"}, {F}, D, false);
    L.fc1_b = B.vec(p + ".mlp.0.bias", F, -0.02f, 0.02f);
    L.fc2 = B.q4({p + ".mlp.2.weight"}, {D}, F, false);
    L.fc2_b = B.vec(p + ".mlp.2.bias", D, -0.02f, 0.02f);
    if (B.st != WQ4_OK) return B.st;
  }
  m->lnp_w = B.vec("encoder.ln_post.weight", D, 0.9f, 1.1f);
  m->lnp_b = B.vec("encoder.ln_post.bias", D, -0.05f, 0.05f);
  m->tok_emb = B.vec("decoder.token_embedding.weight", (int64_t)c.n_vocab * Dt, -lin_scale(Dt), lin_scale(Dt));
  m->dec_pos = B.vec("decoder.positional_embedding", (int64_t)c.n_text_ctx * Dt, -0.02f, 0.02f);
  m->dec.resize(c.n_text_layer);
  for (int i = 0; i < c.n_text_layer; ++i) {
    const std::string p = "decoder.blocks." + std::to_string(i);
    DecLayer& L = m->dec[i];
    L.ln1_w = B.vec(p + ".attn_ln.weight", Dt, 0.9f, 1.1f);
    L.ln1_b = B.vec(p + ".attn_ln.bias", Dt, -0.05f, 0.05f);
    L.qkv = B.q4({p + ".attn.query.weight", p + ".attn.key.weight", p + ".attn.value.weight"}, {Dt, Dt, Dt}, Dt);
    L.qkv_b = B.bias_cat({p + ".attn.query.bias", p + ".attn.key.bias", p + ".attn.value.bias"}, Dt);
    L.out = B.q4({p + ".attn.out.weight"}, {Dt}, Dt);
    L.out_b = B.vec(p + ".attn.out.bias", Dt, -0.02f, 0.02f);
    L.ln2_w = B.vec(p + ".cross_attn_ln.weight", Dt, 0.9f, 1.1f);
    L.ln2_b = B.vec(p + ".cross_attn_ln.bias", Dt, -0.05f, 0.05f);
    L.cq = B.q4({p + ".cross_attn.query.weight"}, {Dt}, Dt);
    L.cq_b = B.vec(p + ".cross_attn.query.bias", Dt, -0.02f, 0.02f);
    // cross-attention key / value (loader.rs:205-210; the key bias, absent
    // in Whisper, cancels in the softmax and is not needed)
    L.ck_raw = B.raw(p + ".cross_attn.key.weight", Dt, D);
    L.cv_raw = B.raw(p + ".cross_attn.value.weight", Dt, D);
    if (L.cv_raw && m->wtype == 0) {
      const size_t nw = wv_pack_words(m->cfg.n_text_head, Dt);
      L.cv_p = m->dev.alloc<uint32_t>(nw);
      if (!L.cv_p || launch_wv_pack(L.cv_raw, m->cfg.n_text_head, Dt, L.cv_p, nullptr) != hipSuccess)
        return fail(WQ4_ENOMEM, "cross-attention Wv repack");
      m->bytes += nw * 4;
    }
    L.cv_b = B.bias_cat({p + ".cross_attn.value.bias"}, Dt);
    if (m->kv_clips > 0) {  // the cache GEMMs run at encoder row counts only: no decode-step copy
      L.ck = B.q4({p + ".cross_attn.key.weight"}, {Dt}, D, false);
      L.cv = B.q4({p + ".cross_attn.value.weight"}, {Dt}, D, false);
    }
    L.cout = B.q4({p + ".cross_attn.out.weight"}, {Dt}, Dt);
    L.cout_b = B.vec(p + ".cross_attn.out.bias", Dt, -0.02f, 0.02f);
    L.ln3_w = B.vec(p + ".mlp_ln.weight", Dt, 0.9f, 1.1f);
    L.ln3_b = B.vec(p + ".mlp_ln.bias", Dt, -0.05f, 0.05f);
    L.fc1 = B.q4({p + ".mlp.0.weight"}, {Ft}, Dt);
    L.fc1_b = B.vec(p + ".mlp.0.bias", Ft, -0.02f, 0.02f);
    L.fc2 = B.q4({p + ".mlp.2.weight"}, {Dt}, Ft);
    L.fc2_b = B.vec(p + ".mlp.2.bias", Dt, -0.02f, 0.02f);
    if (B.st != WQ4_OK) return B.st;
  }
  m->dln_w = B.vec("decoder.ln.weight", Dt, 0.9f, 1.1f);
  m->dln_b = B.vec("decoder.ln.bias", Dt, -0.05f, 0.05f);
  return B.st;
}

// W gamma and W beta + bias of every decoder GEMM that reads a LayerNorm
// (wq4_ln_fold_vectors, double accumulation from the dequantized weights),
// layers spread over host threads.
wq4_status build_ln_fold(wa_model* m) {
  const int Dt = m->cfg.n_text_state;
  struct Job {
    wq4_tensor* w;
    const float *g, *b, *bias;
    float **wg, **b2;
  };
  std::vector<Job> jobs;
  for (DecLayer& L : m->dec) {
    jobs.push_back({L.qkv, L.ln1_w, L.ln1_b, L.qkv_b, &L.qkv_wg, &L.qkv_b2});
    jobs.push_back({L.cq, L.ln2_w, L.ln2_b, L.cq_b, &L.cq_wg, &L.cq_b2});
    jobs.push_back({L.fc1, L.ln3_w, L.ln3_b, L.fc1_b, &L.fc1_wg, &L.fc1_b2});
  }
  for (Job& j : jobs) {
    int64_t n = 0, k = 0;
    (void)wq4_tensor_shape(j.w, &n, &k);
    *j.wg = m->dev.alloc<float>((size_t)n);
    *j.b2 = m->dev.alloc<float>((size_t)n);
    if (!*j.wg || !*j.b2) return fail(WQ4_ENOMEM, "LayerNorm-fold vector allocation failed");
    m->bytes += (size_t)n * 8;
  }
  std::atomic<size_t> next{0};
  std::atomic<int> bad{0};
  auto work = [&]() {
    (void)hipSetDevice(m->device);
    for (size_t i = next++; i < jobs.size(); i = next++) {
      const Job& j = jobs[i];
      int64_t n = 0, k = 0;
      (void)wq4_tensor_shape(j.w, &n, &k);
      std::vector<float> g(Dt), b(Dt), bias((size_t)n), wg((size_t)n), b2((size_t)n);
      if (hipMemcpy(g.data(), j.g, Dt * 4, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(b.data(), j.b, Dt * 4, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(bias.data(), j.bias, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
          wq4_ln_fold_vectors(j.w, g.data(), b.data(), bias.data(), wg.data(), b2.data()) != WQ4_OK ||
          hipMemcpy(*j.wg, wg.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(*j.b2, b2.data(), (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess)
        bad = 1;
    }
  };
  const unsigned nt = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> th;
  for (unsigned t = 0; t < nt; ++t) th.emplace_back(work);
  for (auto& t : th) t.join();
  if (bad) return fail(WQ4_EHIP, "LayerNorm-fold vectors failed");
  return WQ4_OK;
}

}  // namespace wa

extern "C" wq4_status wa_synth_uniform(uint64_t seed, const char* name, int64_t n, float lo, float hi, float* out) {
  if (!name || !out || n < 0) return fail(WQ4_EINVAL, "bad argument");
  synth_uniform(seed, name, n, lo, hi, out);
  return WQ4_OK;
}
