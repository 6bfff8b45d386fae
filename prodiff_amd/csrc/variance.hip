// Encoders of the variance predictors (include/prodiff_hip.h, "variance predictors"):
//
// pd_pitch_cond -- PitchPredictor.forward up to the sampler (modules/variance_predictor/pitch_predictor.py:57-114)
//   fft_embed_tokens  phoneme embedding, extra = dur_embed(mel2ph_to_dur(mel2ph))          :66-70
//   fft_stack         phoneme FastspeechEncoder (width H)
//   note_embed        NoteEncoder.forward_embedding (tts_modules.py:354-365), mask = midi >= 0
//   fft_stack         note encoder (width Hn)
//   GEMM              note_encode_out_linear, Hn -> H                                      :78
//   pitch_combine     both length-regulator gathers + speaker + retake + delta-pitch sums  :72-114
//
// pd_dur -- DurPredictor.forward (dur_predictor.py:31-36)
//   fft_embed_tokens  extra = onset_embed(onset) + word_dur_embed(word_dur)
//   fft_stack         FastspeechEncoder
//   per layer         GEMM (k-tap conv + bias + ReLU) -> LayerNorm(eps 1e-12) * mask       tts_modules.py:119-125
//   dur_head          linear to one value per token, * mask, out2dur + clamp               :126-132
//
// Activations are time-major [batch][token][channel]; everything runs on `stream`, allocation-free.
#include <algorithm>
#include <cmath>

#include "../../include/prodiff_hip.h"
#include "common.h"
#include "fft_stack.h"
#include "gemm.h"
#include "kernels.h"

using namespace pd;

namespace {

// ---------------------------------------------------------------- note embedding
// NoteEncoder.forward_embedding (tts_modules.py:354-365).  One block per (8 notes, utterance):
//  * dur[n] = #{ frames f : mel2note[f] == n+1 }                 (mel2ph_to_dur, pitch_predictor.py:76)
//  * pos[n] = #{ n' <= n : midi[n'] >= 0 } for notes, 0 for padding (make_positions on ~(midi < 0))
//  * x[n,c] = ((sqrt(H) (midi mw[c] + mb[c])) [!rest] + (dur dw[c] + db[c]) + pe(pos, c)) * [midi >= 0]
//  * mask[n] = [midi >= 0]                                        (the encoder's padding mask, :349)
constexpr int NOTE_TOK = 8;

__global__ __launch_bounds__(256) void note_embed_kernel(
    const float* __restrict__ midi, const unsigned char* __restrict__ rest, const long long* __restrict__ mel2note,
    int Tn, int Tm, int H, const float* __restrict__ mw, const float* __restrict__ mb, const float* __restrict__ dw,
    const float* __restrict__ db, float scale, float neg_freq, float* __restrict__ x, int* __restrict__ mask) {
  const int b = blockIdx.y, t0 = blockIdx.x * NOTE_TOK, tid = threadIdx.x;
  __shared__ int cnt[NOTE_TOK];
  __shared__ int npre;
  __shared__ int pos[NOTE_TOK];
  if (tid < NOTE_TOK) cnt[tid] = 0;
  if (tid == 0) npre = 0;
  __syncthreads();
  const float* md = midi + (long long)b * Tn;
  const long long* mp = mel2note + (long long)b * Tm;
  for (int f = tid; f < Tm; f += 256) {
    const long long v = mp[f];
    const long long j = v - 1 - t0;
    if (v >= 1 && v <= Tn && j >= 0 && j < NOTE_TOK) atomicAdd(&cnt[j], 1);
  }
  int pre = 0;
  for (int i = tid; i < t0 && i < Tn; i += 256) pre += md[i] >= 0.f;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) pre += __shfl_xor(pre, o);
  if ((tid & 63) == 0 && pre) atomicAdd(&npre, pre);
  __syncthreads();
  if (tid == 0) {
    int run = npre;
    for (int j = 0; j < NOTE_TOK; ++j) {
      const int t = t0 + j;
      const bool np = t < Tn && md[t] >= 0.f;
      run += np;
      pos[j] = np ? run : 0;
    }
  }
  __syncthreads();
  const int half = H / 2;
  for (int j = 0; j < NOTE_TOK; ++j) {
    const int t = t0 + j;
    if (t >= Tn) break;
    const float m = md[t];
    const bool np = m >= 0.f;
    const float keep = rest[(long long)b * Tn + t] ? 0.f : 1.f;
    const float d = (float)cnt[j];
    const float p = (float)pos[j];
    float* xr = x + ((long long)b * Tn + t) * H;
    if (tid == 0) mask[(long long)b * Tn + t] = np;
    for (int c = tid; c < H; c += 256) {
      const int i = c < half ? c : c - half;
      const float arg = p * expf((float)i * neg_freq);
      const float pe = pos[j] == 0 ? 0.f : (c < half ? sinf(arg) : cosf(arg));
      const float v = ((scale * (m * mw[c] + mb[c])) * keep + (d * dw[c] + db[c])) + pe;
      xr[c] = np ? v : 0.f;
    }
  }
}

// ---------------------------------------------------------------- pitch condition assembly
// pitch_predictor.py:72-114 for one mel frame per wave:
//   cond = ((((pad0(enc)[mel2ph] + pad0(note_lin)[mel2note]) + spk) + retake) + (delta dw + db))
// (F.pad row 0 makes index 0 a zero row; an index past the sequence gathers zero as well).
struct PitchCombineArgs {
  const float* enc;              // [B, Tt, H]
  const float* nlin;             // [B, Tn, H]
  const long long* mel2ph;       // [B, Tm]
  const long long* mel2note;     // [B, Tm]
  const float* spk_tab;          // spk_embed.weight or null
  const long long* spk_id;
  int n_spk;
  const float* E;                // pitch_retake_embed.weight [2, H]
  const float* expr;             // [B] or null
  const unsigned char* retake;   // [B, Tm] or null
  const float* pitch;
  const float* base;
  const float* dw;               // delta_pitch_embed
  const float* db;
  float* out;                    // [B, Tm, H]
  int B, Tt, Tn, Tm, H;
};

__global__ __launch_bounds__(256) void pitch_combine_kernel(const PitchCombineArgs a) {
  const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= (long long)a.B * a.Tm) return;
  const int b = (int)(r / a.Tm);
  float* orow = a.out + r * a.H;
  const long long m = a.mel2ph[r], n = a.mel2note[r];
  const float* er = (m >= 1 && m <= a.Tt) ? a.enc + ((long long)b * a.Tt + (m - 1)) * a.H : nullptr;
  const float* nr = (n >= 1 && n <= a.Tn) ? a.nlin + ((long long)b * a.Tn + (n - 1)) * a.H : nullptr;
  const float* sr = a.spk_tab ? a.spk_tab + min(max(a.spk_id[b], 0ll), (long long)a.n_spk - 1) * a.H : nullptr;
  const int rt = a.retake ? (a.retake[r] != 0) : 1;
  // (pitch - base_pitch) * ~pitch_retake, or zeros without pitch_retake (:109-112)
  const float delta = a.retake ? (a.pitch[r] - a.base[r]) * (rt ? 0.f : 1.f) : 0.f;
  const float e = a.expr ? a.expr[b] * (float)rt : 0.f;
  const float* E0 = a.E;
  const float* E1 = a.E + a.H;
  const float* Er = rt ? E1 : E0;
  for (int c = lane; c < a.H; c += 64) {
    float v = (er ? er[c] : 0.f) + (nr ? nr[c] : 0.f);
    if (sr) v += sr[c];
    v += a.expr ? E1[c] * e + E0[c] * (1.f - e) : Er[c];
    v += delta * a.dw[c] + a.db[c];
    orow[c] = v;
  }
}

// ---------------------------------------------------------------- duration head
// tts_modules.py:126-132, one wave per token: v = (x . w + b) * mask; log_out = v;
// dur_out = max(exp(v) - offset, 0).
__global__ __launch_bounds__(256) void dur_head_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, const int* __restrict__ mask,
                                                       float offset, float* __restrict__ log_out,
                                                       float* __restrict__ dur_out, int rows, int C) {
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (r >= rows) return;
  const float* xr = x + (long long)r * C;
  float s = 0.f;
  for (int c = lane; c < C; c += 64) s += xr[c] * w[c];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) s += __shfl_xor(s, o);
  if (lane) return;
  const float v = mask[r] ? s + bias[0] : 0.f;
  if (log_out) log_out[r] = v;
  if (dur_out) dur_out[r] = fmaxf(expf(v) - offset, 0.f);
}

size_t al64(size_t n) { return (n + 63) / 64 * 64; }

}  // namespace

// ======================================================================= pd_pitch_cond
struct pd_pitch_cond {
  pd_pitch_cond_dims d;
  WeightPool weights;   // every float* below, and the stacks', points into it
  FftStack enc, note;
  float *emb = nullptr, *dur_w = nullptr, *dur_b = nullptr;
  float *mw = nullptr, *mb = nullptr, *ndw = nullptr, *ndb = nullptr;   // note_midi_embed, note_dur_embed
  float *Wol = nullptr, *bol = nullptr;                                 // note_encode_out_linear [H][Hn]
  float *spk = nullptr, *dpw = nullptr, *dpb = nullptr, *E = nullptr;
};

namespace {
struct PitchWs {
  FftWs ph, note;
  size_t enc, nenc, nlin, part, total;
};
PitchWs pitch_ws(const pd_pitch_cond* h, int B, int Tt, int Tn) {
  const size_t Rt = (size_t)B * Tt, Rn = (size_t)B * Tn;
  const int H = h->enc.H, Hn = h->note.H;
  PitchWs w{};
  w.ph = fft_ws(h->enc, Rt, 0);
  w.note = fft_ws(h->note, Rn, w.ph.end);
  size_t o = w.note.end;
  w.enc = o; o += al64(Rt * H);
  w.nenc = o; o += al64(Rn * Hn);
  w.nlin = o; o += al64(Rn * H);
  w.part = o; o += al64(enc_part_floats(Rn, H, Hn));
  w.total = o * sizeof(float);
  return w;
}
}  // namespace

extern "C" {

int pd_pitch_cond_num_params(const pd_pitch_cond_dims* d) {
  if (!d) return -1;
  return (10 * d->enc_layers + 2) + 1 + 2 + (10 * d->note_layers + 2) + 4 + 2 + !!d->use_spk_id + 2 + 1;
}

int pd_pitch_cond_create(const pd_pitch_cond_dims* dims, const float* const* params, int dtype, void* stream,
                         pd_pitch_cond** out) {
  PD_CHECK_ARG(dims && out, "null pointer");
  const pd_pitch_cond_dims& d = *dims;
  PD_CHECK_ARG(dtype == PD_DTYPE_F32 || dtype == PD_DTYPE_BF16, "dtype must be PD_DTYPE_F32 or PD_DTYPE_BF16");
  {
    FftStack probe;
    PD_TRY(probe.init(d.hidden_size, d.enc_layers, d.enc_ffn_kernel_size, d.num_heads, "pd_pitch_cond encoder"));
    PD_TRY(probe.init(d.note_hidden_size, d.note_layers, d.note_ffn_kernel_size, d.note_heads,
                      "pd_pitch_cond note encoder"));
  }
  PD_CHECK_ARG(d.vocab_size > 0, "bad vocab_size");
  PD_CHECK_ARG(!d.use_spk_id || d.num_spk > 0, "num_spk must be positive with use_spk_id");
  PD_CHECK_ARG(params, "null pointer");
  PD_TRY(check_params(params, pd_pitch_cond_num_params(dims)));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_pitch_cond> h(new pd_pitch_cond());
  h->d = d;
  h->enc.init(d.hidden_size, d.enc_layers, d.enc_ffn_kernel_size, d.num_heads, "pd_pitch_cond");   // checked above
  h->note.init(d.note_hidden_size, d.note_layers, d.note_ffn_kernel_size, d.note_heads, "pd_pitch_cond");
  const int H = h->enc.H, Hn = h->note.H;
  const size_t V = (size_t)d.vocab_size + 1;
  WeightPool& wp = h->weights;
  ParamView pv{params, pd_pitch_cond_num_params(dims)};
  h->enc.add_to(wp, pv);
  wp.add_copy(&h->emb, V * H, pv.next());
  wp.add_copy(&h->dur_w, H, pv.next());
  wp.add_copy(&h->dur_b, H, pv.next());
  h->note.add_to(wp, pv);
  wp.add_copy(&h->mw, Hn, pv.next());
  wp.add_copy(&h->mb, Hn, pv.next());
  wp.add_copy(&h->ndw, Hn, pv.next());
  wp.add_copy(&h->ndb, Hn, pv.next());
  wp.add_copy(&h->Wol, (size_t)H * Hn, pv.next());   // [H, Hn] = W[n][k]
  wp.add_copy(&h->bol, H, pv.next());
  if (d.use_spk_id) wp.add_copy(&h->spk, (size_t)d.num_spk * H, pv.next());
  wp.add_copy(&h->dpw, H, pv.next());
  wp.add_copy(&h->dpb, H, pv.next());
  wp.add_copy(&h->E, (size_t)2 * H, pv.next());
  PD_TRY(pv.done("pd_pitch_cond"));
  PD_TRY(wp.commit(st, "pitch-condition"));
  if (dtype == PD_DTYPE_BF16) PD_TRY(wp.mirror_bf16(st));
  *out = h.release();
  return PD_OK;
}

void pd_pitch_cond_destroy(pd_pitch_cond* h) { delete h; }

size_t pd_pitch_cond_workspace_size(const pd_pitch_cond* h, int B, int T_txt, int T_note, int T_mel) {
  if (!h || B < 1 || T_txt < 1 || T_note < 1 || T_mel < 1) return 0;
  return pitch_ws(h, B, T_txt, T_note).total;
}

int pd_pitch_cond_forward(const pd_pitch_cond* h, const pd_pitch_cond_inputs* in, float* cond, int B, int T_txt,
                          int T_note, int T_mel, void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && in && cond && workspace, "null pointer");
  PD_CHECK_ARG(B > 0 && T_txt > 0 && T_note > 0 && T_mel > 0, "bad B / T_txt / T_note / T_mel");
  PD_CHECK_ARG(in->txt_tokens && in->mel2ph, "txt_tokens and mel2ph are required");
  PD_CHECK_ARG(in->note_midi && in->note_rest && in->mel2note, "note_midi, note_rest and mel2note are required");
  const pd_pitch_cond_dims& d = h->d;
  if (d.use_spk_id) PD_CHECK_ARG(in->spk_id, "use_spk_id: spk_id is required");
  if (in->pitch_retake) PD_CHECK_ARG(in->pitch && in->base_pitch, "pitch_retake: pitch and base_pitch are required");
  const PitchWs w = pitch_ws(h, B, T_txt, T_note);
  if (ws_bytes < w.total) { set_error("workspace too small"); return PD_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const int H = h->enc.H, Hn = h->note.H;
  float* enc = ws + w.enc;
  float* nenc = ws + w.nenc;
  float* nlin = ws + w.nlin;
  {
    TokEmbedArgs e{};
    e.tok = in->txt_tokens; e.mel2ph = in->mel2ph;
    e.Tt = T_txt; e.Tm = T_mel; e.H = H; e.emb = h->emb; e.V = d.vocab_size + 1;
    e.dur_w = h->dur_w; e.dur_b = h->dur_b;
    e.x = ws + w.ph.x; e.mask = reinterpret_cast<int*>(ws + w.ph.mask);
    PD_TRY(fft_embed_tokens(e, B, st));
  }
  PD_TRY(fft_stack_forward<U_PITCH_PH_BASE>(h->enc, ws, w.ph, in->txt_lens, enc, B, T_txt, st));
  {
    ProfScope ps("note_embed", st);
    hipLaunchKernelGGL(note_embed_kernel, dim3(cdiv(T_note, NOTE_TOK), B), dim3(256), 0, st, in->note_midi,
                       in->note_rest, in->mel2note, T_note, T_mel, Hn, h->mw, h->mb, h->ndw, h->ndb,
                       (float)std::sqrt((double)Hn), (float)(-(std::log(10000.0) / (Hn / 2 - 1))), ws + w.note.x,
                       reinterpret_cast<int*>(ws + w.note.mask));
  }
  PD_LAUNCH_CHECK();
  PD_TRY(fft_stack_forward<U_PITCH_NOTE_BASE>(h->note, ws, w.note, in->note_lens, nenc, B, T_note, st));
  {   // note_encode_out_linear (pitch_predictor.py:78)
    const long long bs = (long long)T_note;
    GemmArgs a = make_gemm(B, T_note, H, h->Wol, Hn, h->bol, nlin, bs * H, H);
    add_seg(a, make_seg(nenc, bs * Hn, Hn, Hn, 0));
    PD_TRY((enc_gemm<EPI_STORE, U_PITCH_NOTE_OUT>(a, ws + w.part, st, "pitch_note_out")));
  }
  PitchCombineArgs a{};
  a.enc = enc; a.nlin = nlin; a.mel2ph = in->mel2ph; a.mel2note = in->mel2note;
  if (d.use_spk_id) { a.spk_tab = h->spk; a.spk_id = in->spk_id; a.n_spk = d.num_spk; }
  a.E = h->E; a.expr = in->pitch_expr; a.retake = in->pitch_retake; a.pitch = in->pitch; a.base = in->base_pitch;
  a.dw = h->dpw; a.db = h->dpb; a.out = cond;
  a.B = B; a.Tt = T_txt; a.Tn = T_note; a.Tm = T_mel; a.H = H;
  {
    ProfScope ps("pitch_combine", st);
    hipLaunchKernelGGL(pitch_combine_kernel, dim3(cdiv((long long)B * T_mel, 4)), dim3(256), 0, st, a);
  }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"

// ======================================================================= pd_dur
struct pd_dur {
  pd_dur_dims d;
  WeightPool weights;
  FftStack enc;
  float *emb = nullptr, *onset = nullptr, *wdw = nullptr, *wdb = nullptr;
  std::vector<float*> Wc, bc, lng, lnb;   // per DurationPredictor layer: conv W[C][k*Cin], bias, LayerNorm
  float *lw = nullptr, *lb = nullptr;     // linear [1, C], [1]
};

namespace {
struct DurWs {
  FftWs s;
  size_t enc, a, b, part, total;
};
DurWs dur_ws(const pd_dur* h, int B, int Tt) {
  const size_t R = (size_t)B * Tt;
  const int H = h->enc.H, C = h->d.n_chans, k = h->d.kernel_size;
  DurWs w{};
  w.s = fft_ws(h->enc, R, 0);
  size_t o = w.s.end;
  w.enc = o; o += al64(R * H);
  w.a = o; o += al64(R * C);
  w.b = o; o += al64(R * C);
  w.part = o; o += al64(std::max(enc_part_floats(R, C, k * H), enc_part_floats(R, C, k * C)));
  w.total = o * sizeof(float);
  return w;
}
}  // namespace

extern "C" {

int pd_dur_num_params(const pd_dur_dims* d) {
  if (!d) return -1;
  return (10 * d->enc_layers + 2) + 1 + 1 + 2 + 4 * d->n_layers + 2;
}

int pd_dur_create(const pd_dur_dims* dims, const float* const* params, int dtype, void* stream, pd_dur** out) {
  PD_CHECK_ARG(dims && out, "null pointer");
  const pd_dur_dims& d = *dims;
  PD_CHECK_ARG(dtype == PD_DTYPE_F32 || dtype == PD_DTYPE_BF16, "dtype must be PD_DTYPE_F32 or PD_DTYPE_BF16");
  {
    FftStack probe;
    PD_TRY(probe.init(d.hidden_size, d.enc_layers, d.enc_ffn_kernel_size, d.num_heads, "pd_dur encoder"));
  }
  PD_CHECK_ARG(d.vocab_size > 0, "bad vocab_size");
  PD_CHECK_ARG(d.n_layers >= 1, "n_layers must be >= 1");
  PD_CHECK_ARG(d.n_chans > 0 && d.n_chans % GEMM_BK == 0, "n_chans must be a positive multiple of 32");
  PD_CHECK_ARG(d.kernel_size > 0 && d.kernel_size % 2 == 1 && d.kernel_size <= MAX_SEGS,
               "kernel_size must be odd and <= 11 (SAME padding)");
  PD_CHECK_ARG(params, "null pointer");
  PD_TRY(check_params(params, pd_dur_num_params(dims)));
  hipStream_t st = (hipStream_t)stream;
  std::unique_ptr<pd_dur> h(new pd_dur());
  h->d = d;
  h->enc.init(d.hidden_size, d.enc_layers, d.enc_ffn_kernel_size, d.num_heads, "pd_dur");   // checked above
  const int H = h->enc.H, C = d.n_chans, k = d.kernel_size, NL = d.n_layers;
  WeightPool& wp = h->weights;
  ParamView pv{params, pd_dur_num_params(dims)};
  h->enc.add_to(wp, pv);
  wp.add_copy(&h->emb, (size_t)d.vocab_size * H, pv.next());
  wp.add_copy(&h->onset, (size_t)2 * H, pv.next());
  wp.add_copy(&h->wdw, H, pv.next());
  wp.add_copy(&h->wdb, H, pv.next());
  h->Wc.resize(NL); h->bc.resize(NL); h->lng.resize(NL); h->lnb.resize(NL);
  for (int l = 0; l < NL; ++l) {
    const int Cin = l ? C : H;
    wp.add_conv(&h->Wc[l], pv.next(), C, Cin, k, Cin);   // conv.l.1 [C, Cin, k]
    wp.add_copy(&h->bc[l], C, pv.next());
    wp.add_copy(&h->lng[l], C, pv.next());
    wp.add_copy(&h->lnb[l], C, pv.next());
  }
  wp.add_copy(&h->lw, C, pv.next());
  wp.add_copy(&h->lb, 1, pv.next());
  PD_TRY(pv.done("pd_dur"));
  PD_TRY(wp.commit(st, "duration-predictor"));
  if (dtype == PD_DTYPE_BF16) PD_TRY(wp.mirror_bf16(st));
  *out = h.release();
  return PD_OK;
}

void pd_dur_destroy(pd_dur* h) { delete h; }

size_t pd_dur_workspace_size(const pd_dur* h, int B, int T_txt) {
  if (!h || B < 1 || T_txt < 1) return 0;
  return dur_ws(h, B, T_txt).total;
}

int pd_dur_forward(const pd_dur* h, const pd_dur_inputs* in, float* log_out, float* dur_out, int B, int T_txt,
                   void* workspace, size_t ws_bytes, void* stream) {
  PD_CHECK_ARG(h && in && workspace, "null pointer");
  PD_CHECK_ARG(B > 0 && T_txt > 0, "bad B / T_txt");
  PD_CHECK_ARG(in->txt_tokens && in->onset && in->word_dur, "txt_tokens, onset and word_dur are required");
  PD_CHECK_ARG(log_out || dur_out, "nothing to write: log_out and dur_out are both null");
  const DurWs w = dur_ws(h, B, T_txt);
  if (ws_bytes < w.total) { set_error("workspace too small"); return PD_ERR_WORKSPACE; }
  hipStream_t st = (hipStream_t)stream;
  float* ws = (float*)workspace;
  const pd_dur_dims& d = h->d;
  const int H = h->enc.H, C = d.n_chans, k = d.kernel_size;
  const int rows = B * T_txt;
  const long long bs = (long long)T_txt;
  const int* mask = reinterpret_cast<const int*>(ws + w.s.mask);
  float* enc = ws + w.enc;
  float* ya = ws + w.a;
  float* yb = ws + w.b;
  {
    TokEmbedArgs e{};
    e.tok = in->txt_tokens;
    e.Tt = T_txt; e.Tm = 0; e.H = H; e.emb = h->emb; e.V = d.vocab_size;
    e.onset = in->onset; e.onset_emb = h->onset; e.word_dur = in->word_dur; e.wd_w = h->wdw; e.wd_b = h->wdb;
    e.x = ws + w.s.x; e.mask = reinterpret_cast<int*>(ws + w.s.mask);
    PD_TRY(fft_embed_tokens(e, B, st));
  }
  PD_TRY(fft_stack_forward<U_DUR_ENC_BASE>(h->enc, ws, w.s, in->txt_lens, enc, B, T_txt, st));
  // The conv input is zero on padding tokens (the encoder's final mask, then each layer's own), which is the
  // zero padding of the row alone: the convs need no lens.
  const float* src = enc;
  for (int l = 0; l < d.n_layers; ++l) {
    const int Cin = l ? C : H;
    GemmArgs a = make_gemm(B, T_txt, C, h->Wc[l], k * Cin, h->bc[l], ya, bs * C, C);
    for (int tap = 0; tap < k; ++tap) add_seg(a, make_seg(src, bs * Cin, Cin, Cin, tap - k / 2));
    a.act = ACT_RELU;
    PD_TRY((enc_gemm<EPI_STORE, U_DUR_CONV>(a, ws + w.part, st, "dur_conv")));
    PD_TRY(fft_layer_norm(ya, h->lng[l], h->lnb[l], mask, yb, rows, C, 1e-12f, 1, st));
    src = yb;
  }
  {
    ProfScope ps("dur_head", st);
    hipLaunchKernelGGL(dur_head_kernel, dim3(cdiv(rows, 4)), dim3(256), 0, st, src, h->lw, h->lb, mask,
                       d.log_offset, log_out, dur_out, rows, C);
  }
  PD_LAUNCH_CHECK();
  return PD_OK;
}

}  // extern "C"
