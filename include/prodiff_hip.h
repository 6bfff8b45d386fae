/*
 * prodiff_hip.h -- C-ABI of libprodiff_hip.so, the MI355X (gfx950) ProDiff/FastDiff
 * inference hot path.
 *
 * Conventions
 *  - Every tensor pointer is a caller-owned DEVICE buffer (e.g. torch.cuda tensors),
 *    float32, contiguous, 16-byte aligned.  Host pointers appear only where a
 *    parameter is documented as "host" (per-step scalars).
 *  - Calls are asynchronous and stream-ordered on `stream` (a hipStream_t; NULL =
 *    the default stream).  Nothing allocates or synchronises inside forward/sample
 *    calls, so they can be captured into a hipGraph.  Scratch memory is passed in
 *    (`workspace`, at least *_workspace_size() bytes).
 *  - Handles are immutable after create; concurrent calls on different streams
 *    need separate workspaces.
 *  - Return 0 (PD_OK) or an error code; pd_last_error() gives a thread-local text.
 *    Argument checks mirror the reference's assert points (e.g. the LVC length
 *    check, modules/FastDiff/module/modules.py:236).
 *  - Layouts: "time-major" = [batch][time][channel] (channels contiguous), the
 *    layout ProDiff's condition/mel already have at the sampler boundary
 *    (prodiff.py:136-138 receives cond [B,T,H]; :151 returns mel [B,T,M]).
 *    "channel-major" = PyTorch Conv1d layout [batch][channel][time].
 *    The 2-D networks (pitch extraction, harmonic-noise separation) keep channels-last
 *    images [batch][frame][bin][channel] inside; spectra cross the boundary as planar
 *    re / im arrays [row][frame][bin].
 */
#ifndef PRODIFF_HIP_H
#define PRODIFF_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PD_OK 0
#define PD_ERR_ARG 1
#define PD_ERR_HIP 2
#define PD_ERR_WORKSPACE 3
#define PD_ERR_UNSUPPORTED 4

#define PD_DTYPE_F32 0
#define PD_DTYPE_BF16 1

const char* pd_last_error(void);
int pd_version(void);
/* "default" for the shipped build; otherwise the non-default compile-time knobs it was built with
 * (A/B variant libraries, tools/build_variant_lib.sh).  bench.py records it; the GPU tests refuse a
 * variant library unless PRODIFF_ALLOW_VARIANT=1. */
const char* pd_build_config(void);
/* Device bytes held by the live handles of this process (weight pools, their bf16 mirrors and
 * the handles' other allocations); 0 once every handle is destroyed. */
size_t pd_live_device_bytes(void);

/* Per-launch timing for benchmarks: when enabled, HIP events are recorded on the
 * launch stream around every hot-path kernel (tagged by use, e.g. "fd_kp_kernel").
 * pd_profile_enable(1) also clears previous records.  pd_profile_summary waits
 * for the recorded events and writes "tag count total_ms" lines; it returns the
 * buffer size needed (including the NUL), or -1 on error. */
int pd_profile_enable(int on);
int pd_profile_summary(char* buf, int buflen);
/* Restrict recording to the tags in a comma-separated list (NULL or "" = every tag).
 * An event pair costs GPU time at every launch it brackets; bench.py times its step with
 * only the dominant kernel recorded. */
int pd_profile_filter(const char* tags);

/* ===================================================================== ProDiff
 * WaveNet denoiser -- replaces modules/decoder/wavenet.py:74-123 (WaveNet) as the
 * `denoise_fn` of GaussianDiffusion (modules/diffusion/prodiff.py:49-54,125).
 */
typedef struct pd_wavenet pd_wavenet;

typedef struct {
  int in_dims;               /* M: mel bins (80 LJSpeech, 128 SVS)          wavenet.py:75 */
  int hidden_size;           /* H: condition channels (encoder_hidden)                   */
  int residual_layers;       /* L: 20 (handler/base_config.yaml:210)                     */
  int residual_channels;     /* C: 256 (base_config.yaml:211), multiple of 32            */
  int dilation_cycle_length; /* dilation 2^(l % cycle) (wavenet.py:93-96); min(L, cycle) <= 31 */
} pd_wavenet_dims;

/* Parameter order = the reference state-dict order (wavenet.py:84-99), all float32
 * in their PyTorch shapes:
 *   input_projection.{weight[C,M,1],bias[C]}, mlp.0.{weight[4C,C],bias},
 *   mlp.2.{weight[C,4C],bias},
 *   for l < L: residual_layers.l.{dilated_conv.weight[2C,C,3], dilated_conv.bias,
 *              diffusion_projection.weight[C,C], diffusion_projection.bias,
 *              conditioner_projection.weight[2C,H,1], conditioner_projection.bias,
 *              output_projection.weight[2C,C,1], output_projection.bias},
 *   skip_projection.{weight[C,C,1],bias}, output_projection.{weight[M,C,1],bias}. */
#define PD_WAVENET_NUM_PARAMS(L) (6 + 8 * (L) + 4)

/* Packs the weights into the kernels' layouts (device-to-device, on `stream`). */
int pd_wavenet_create(const pd_wavenet_dims* dims, const float* const* params, int dtype,
                      void* stream, pd_wavenet** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_wavenet_destroy(pd_wavenet* h);
/* Kernel-variant option of a handle; set before its first call.  PD_WN_OPT_LAYER selects the
 * bf16 residual-layer implementation: 0 the fused kernel with 32-frame blocks, 3 the fused
 * kernel with 64-frame blocks, 2 (default) 64-frame fused blocks when they still give every CU a
 * block (B*T >= 16384 frames) else 32.  DESIGN.md §4 has the measurements.
 * 1: reserved (r02's two launches per layer, GATE + RESSKIP kernels, removed: measured slower,
 * DESIGN.md §4) -- PD_ERR_ARG. */
#define PD_WN_OPT_LAYER 0
/* PD_WN_OPT_KSPLIT (fp32 path): the residual-layer GEMMs split their K range over several blocks
 * until the grid holds 512 (default) or 256 blocks; 0 = never split. */
#define PD_WN_OPT_KSPLIT 1
/* PD_WN_OPT_L2PF (bf16 fused layer): 1 (default) each layer launch pulls the next layer's weight
 * fragments into every XCD's L2 while it runs; 0 = off. */
#define PD_WN_OPT_L2PF 2
/* PD_WN_OPT_STACK (bf16, C = H = 256, every dilation <= 16 -- min(L, dilation_cycle_length) <= 5 --, L <= 64,
 * T >= 64, PD_WN_OPT_LAYER 2; other nets take the one-layer kernel whatever the value): n = 1..16
 * residual layers per launch (wn_stack_bf16_kernel: a 64-frame window per 32 output frames stays
 * resident for the n layers; bit-identical to the one-layer kernel), default 10; 0 = one launch
 * per layer. */
#define PD_WN_OPT_STACK 3
/* PD_WN_OPT_STACK_RO: output frames per wn_stack_bf16_kernel block, 16..48, capped at 64 - 2 max(nl, 8)
 * (the 64-frame window less a halo of one frame per layer each side); 0 (default) = that cap (44 at
 * the default 10 layers per launch). */
#define PD_WN_OPT_STACK_RO 4
/* 5: reserved (r04's in-kernel split-K reduction by arrival counters, removed: measured slower) */
/* PD_WN_OPT_STACK_FUSE (bf16 stack path): 1 (default) the input projection runs inside the first
 * stack launch and, in pd_prodiff_sample, the skip head + output projection + posterior update
 * inside the last one (same roundings and k order as the separate launches); 0 = separate launches. */
#define PD_WN_OPT_STACK_FUSE 6
/* PD_WN_OPT_F32_LAYER (fp32 path): 1 (default) residual layers whose GEMMs would split K (small
 * batches, e.g. B = 1) run as two launches of 32-frame x 32-channel-pair blocks with no split-K
 * partials (wn_f32_layer_kernel); 2 = always; 0 = the split-K GEMM engine. */
#define PD_WN_OPT_F32_LAYER 7
int pd_wavenet_set_option(pd_wavenet* h, int option, int value);
/* S = number of reverse steps the workspace must serve (1 for pd_wavenet_forward). */
size_t pd_wavenet_workspace_size(const pd_wavenet* h, int B, int T, int S);

/* One denoiser call, reference signature WaveNet.forward(spec, diffusion_step, cond)
 * (wavenet.py:100-123):
 *   spec  [B,1,M,T] channel-major, steps [B] (float; integer steps as floats),
 *   cond  [B,H,T] channel-major  ->  out [B,1,M,T]. */
int pd_wavenet_forward(const pd_wavenet* h, const float* spec, const float* steps,
                       const float* cond, float* out, int B, int T, void* workspace,
                       size_t ws_bytes, void* stream);

/* Ragged batches (every sampler below, and nsf_forward): `lens` is a device array of B ints, the
 * length of each row's utterance in mel frames (1 <= lens[b] <= T), or NULL (every row is T frames).
 * Rows stay laid out at the padded length T; frames t >= lens[b] are padding, and every convolution
 * of the network reads them as its zero padding -- so row b's first lens[b] frames (and samples)
 * equal a run of that utterance alone (B = 1, T = lens[b]), the reference's one-segment-at-a-time
 * inference (handler/infer/handler.py:373-388).  Outputs in the padding are unspecified.  With the
 * on-device draws below, the draws of an utterance's frames are the same padded or alone.  A few
 * A/B kernel variants do not take lens (FD_OPT_LVC_TS 0, FD_OPT_KP_CHUNK)
 * and return PD_ERR_UNSUPPORTED. */
/* Random draws (every sampler below).  When the caller passes no explicit draws they come
 * from an on-device Philox4x32-10 generator keyed by (seed, utterance id, element index
 * within the utterance, stream): `utt_ids` is a device array of B ints (one id per batch
 * row) or NULL (ids 0..B-1).  An utterance's output therefore depends on (seed, its id) only,
 * not on its row in the batch or on how a job is sharded over GPUs. */
/* The whole x0-predict reverse sampler, GaussianDiffusion.forward(cond, infer=True)
 * (prodiff.py:136-153) for S = clip(infer_step, 1, timesteps) steps:
 *   x ~ U[0,1); for i = S-1..0: x0 = WaveNet(x, i, cond);
 *   x = coef1[i]*x0 + coef2[i]*x + [i>0]*sigma[i]*n_i
 * with coef1/coef2 = posterior_mean_coef1/2 and sigma = exp(0.5*posterior_log_variance_clipped)
 * (host arrays of length >= S, taken from the checkpoint buffers).
 *   cond  [B,T,H] time-major (as the teacher hands it, prodiff_teacher.py:167)
 *   x_T   [B,T,M] time-major draw, or NULL -> Philox U[0,1) from `seed`
 *   noise [S][B,T,M] time-major draws (pass j uses noise[j]), or NULL -> Philox N(0,1)
 *   mel   [B,T,M] output (the reference's x[:,0].transpose(1,2), prodiff.py:151). */
int pd_prodiff_sample(const pd_wavenet* h, const float* cond, const float* coef1,
                      const float* coef2, const float* sigma, int S, const float* x_T,
                      const float* noise, unsigned long long seed, const int* utt_ids, const int* lens,
                      float* mel, int B, int T, void* workspace, size_t ws_bytes, void* stream);

/* ============================================================= rectified flow
 * RectifiedFlow / PitchRectifiedFlow inference (modules/diffusion/reflow.py:5-144) with
 * the WaveNet velocity field -- the SVS teacher's diff_type "reflow"
 * (modules/svs/prodiff_teacher.py:67-82) and the pitch predictor's sampler
 * (modules/variance_predictor/pitch_predictor.py:40-55):
 *   x ~ N(0,1); dt = 1/max(1,S); for i < S: x = step(x, t = i*dt)      (reflow.py:86-101)
 *   v(x, t) = WaveNet(x, time_scale*t, cond); step = euler / rk2 / rk4 / rk5 (reflow.py:48-84).
 * Euler's update is fused into the velocity output projection. */
#define PD_REFLOW_EULER 0
#define PD_REFLOW_RK2 1
#define PD_REFLOW_RK4 2
#define PD_REFLOW_RK5 3

/* 0 if the arguments are invalid (S * stages > 128, unknown algorithm). */
size_t pd_reflow_workspace_size(const pd_wavenet* h, int B, int T, int S, int algo);

/*   cond [B,T,H] time-major (the condition before the transpose at reflow.py:33)
 *   x_T  [B,T,M] time-major draw, or NULL -> Philox N(0,1) from `seed`
 *   x    [B,T,M] output: the reference's x.transpose(2,3).squeeze(1) before denorm_spec. */
int pd_reflow_sample(const pd_wavenet* h, const float* cond, int S, int algo, float time_scale,
                     const float* x_T, unsigned long long seed, const int* utt_ids, const int* lens, float* x,
                     int B, int T, void* workspace, size_t ws_bytes, void* stream);

/* denorm_spec (reflow.py:106-107): y = (x+1)/2 * (spec_max - spec_min) + spec_min with
 * spec_min/spec_max device arrays of length nspec (1, broadcast, or M);  x [rows,M].
 * mean_clamp = 0: out [rows,M] = y.  mean_clamp = 1 (PitchRectifiedFlow, :138-144):
 * out [rows] = clamp(mean over the M bins of y, clamp_min, clamp_max). */
int pd_reflow_denorm(const float* x, const float* spec_min, const float* spec_max, int nspec, int M,
                     int rows, int mean_clamp, float clamp_min, float clamp_max, float* out,
                     void* stream);

/* ==================================================================== FastDiff
 * eps-network -- replaces modules/FastDiff/module/FastDiff_model.py:10-102 (FastDiff)
 * and the sampler util.py:158-232 (sampling_given_noise_schedule, ddim=False).
 */
typedef struct fd_model fd_model;

typedef struct {
  int audio_channels;        /* 1    (modules/FastDiff/config/base.yaml:20) */
  int inner_channels;        /* 32   */
  int cond_channels;         /* 80   */
  int num_blocks;            /* len(upsample_ratios) = 3 */
  int upsample_ratios[4];    /* 8, 8, 4 (hop 256) */
  int lvc_layers_each_block; /* 4    */
  int lvc_kernel_size;       /* 3    */
  int kpnet_hidden_channels; /* 64   */
  int kpnet_conv_size;       /* 3    */
  int step_embed_in;         /* 128  */
  int step_embed_mid;        /* 512  */
  int step_embed_out;        /* 512  */
} fd_dims;

/* Parameter order (weight-norm already folded, w = g*v/||v||, FastDiff_model.py:104-113;
 * fd_fold_weight_norm does it on device): for every Conv1d "weight" then "bias":
 *   first_audio_conv, fc_t1.{weight,bias}, fc_t2.{weight,bias},
 *   for n < num_blocks (lvc_blocks.n): upsample.{weight[32,32,2r],bias},
 *       kernel_predictor.input_conv.0, kernel_predictor.residual_conv.{1,3,6,8,11,13},
 *       kernel_predictor.kernel_conv, kernel_predictor.bias_conv, fc_t.{weight,bias},
 *       convs.{0..3},
 *   for n < num_blocks (downsample.n): residual_dense, conv.{0,1,2},
 *   final_conv.0. */
#define FD_NUM_PARAMS(nb) (2 + 4 + 30 * (nb) + 8 * (nb) + 2)

int fd_create(const fd_dims* dims, const float* const* params, int dtype, void* stream,
              fd_model** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void fd_destroy(fd_model* m);
int fd_hop(const fd_model* m);   /* prod(upsample_ratios) = samples per mel frame */
/* Workspace of fd_forward (S = 1) or fd_sample (S = N steps; bounded: steps run in chunks of
 * 16, so the 200- and 1000-step schedules of fastdiff.py:58-61 need the 16-step size). */
size_t fd_workspace_size(const fd_model* m, int B, int Tc, int S);

/* Kernel-variant options of a handle (bf16 LVC-block tiling and fusions).  The defaults are
 * the measured production configuration; the tests select each variant.
 * Set them before the handle's first forward/sample call; not thread-safe against calls. */
#define FD_OPT_LVC_TS 0       /* whole-block LVC tile, hop >= 32: 384 (default), 256, 128 (the hop < 32 block: 256);
                               * 0 = per-layer launches */
/* 1: reserved (FD_OPT_LVC_TS_SUB, the hop < 32 block's 128 / 384 tiles, removed: measured slower, r03 A/B at
 * fastdiff.hip's fd_model) */
#define FD_OPT_LVC_FUSE 2     /* 1: upsample / first conv / sampler update fused into the LVC blocks */
#define FD_OPT_LVC_PF 3       /* 1: next-layer kernel fragments prefetched into registers (tile 384) */
#define FD_OPT_LVC_SUB 4      /* 1: the hop < 32 block on the whole-block kernel too */
/* 5: reserved (FD_OPT_KP_SIDE, fd_sample's kernel-predictor GEMMs on a low-priority side stream, removed:
 * measured slower, r01 ab_v16b 7.41 vs 7.33 ms/step) */
/* 6: reserved (r02's streaming LVC kernel, removed in r03: measured slower) */
#define FD_OPT_KP_CHUNK 7     /* n > 0: kernel predictor + LVC block per chunk of n utterances (default 0 = whole batch) */
/* 8, 9: reserved (r03's skewed persistent LVC kernel, removed: measured slower) */
#define FD_OPT_LVC_TPW 10     /* 32-row tiles per wave of the 384-sample hop >= 32 LVC blocks: 2 (8 waves) or 1 (16 waves) */
#define FD_OPT_LVC_PRIO 11    /* 1: s_setprio(1) for the second half of an LVC block's waves */
/* 12: reserved (r04's persistent LVC kernel with LDS-DMA prefetch, removed: measured slower) */
#define FD_OPT_LVC_PS 14      /* 1 (r06): the final (fused, prefetching, 384-sample) LVC block as a persistent kernel whose
                               * next tile's audio / x_prev / biases arrive by LDS-DMA under the current tile's layers */
/* 13: reserved (r04's multi-tile fused-DBlock blocks, removed: measured slower) */
#define FD_OPT_LVC_CARRY 15   /* 1 (default): a persistent LVC block walks runs of consecutive tiles of one utterance and
                               * carries the left halo from tile to tile (448 output rows per 512-row window
                               * instead of 384); 0: 384-row tiles v, v + grid, ... with both halos recomputed */
#define FD_OPT_LVC_PS_GRID 16 /* n > 0: at most n blocks in a persistent LVC launch (default 0 = one per CU) */
int fd_set_option(fd_model* m, int option, int value);

/* The run partition of a persistent LVC launch (FD_OPT_LVC_CARRY) over `batch` utterances of `rows` rows (a
 * multiple of 64) on `grid` blocks: *nruns = the number of runs (0: no more 384-row tiles than blocks, every
 * block takes one tile and nothing is carried), and runs[3 i ..] = (utterance, first row, end row) of run i
 * for i < min(*nruns, cap) (runs may be NULL).  Block v walks runs v, v + grid, ...; a run's first tile yields
 * 384 rows (448 at row 0), every later one 448. */
int fd_lvc_ps_partition(int rows, int batch, int grid, int* runs, int cap, int* nruns);

/* w[co,:] = g[co] * v[co,:] / ||v[co,:]||  (torch.nn.utils.weight_norm, dim 0). */
int fd_fold_weight_norm(float* w, const float* g, const float* v, int cout, int per_row,
                        void* stream);

/* One network call, reference net((audio, c, steps)) (FastDiff_model.py:74-102):
 *   audio [B,1,L] (L = Tc*hop), cond [B,80,Tc] channel-major, steps [B] float
 *   -> eps [B,1,L]. */
int fd_forward(const fd_model* m, const float* audio, const float* cond, const float* steps,
               float* eps, int B, int Tc, void* workspace, size_t ws_bytes, void* stream);

/* sampling_given_noise_schedule(net, (B,1,L), dh, schedule, condition) (util.py:158-232):
 *   x ~ N(0,1); for n = N-1..0: x = (x - beta[n]/sqrt(1-alpha[n]^2) eps(x,c,steps[n]))
 *                                     / sqrt(1-beta[n]) + [n>0] sigma[n] z
 *   mel   [B,Tc,80] time-major (the ProDiff sampler's output, no transpose needed)
 *   beta/alpha/sigma/steps: host arrays of length N (util.py:181-206)
 *   x_T   [B,L] draw or NULL -> Philox N(0,1); noise [N-1][B,L] (pass j uses noise[j])
 *   or NULL -> Philox;  wav [B,L] output. */
int fd_sample(const fd_model* m, const float* mel, const float* beta, const float* alpha,
              const float* sigma, const float* steps, int N, const float* x_T,
              const float* noise, unsigned long long seed, const int* utt_ids, const int* lens, float* wav,
              int B, int Tc, void* workspace, size_t ws_bytes, void* stream);

/* The same reverse process with the per-pass update given directly: pass j (j < N, sampling
 * order) evaluates eps at step value steps[j] and sets x = (x - ce[j] eps) / den[j] + sg[j] z.
 * fd_sample is this with DDPM coefficients (util.py:222-226); DDIM (util.py:215-220,
 * ddim=True) is ce = -(c2 + c3) / c1, den = 1 / c1, sg = 0.  `draw0` offsets the passes'
 * Philox stream ids (a sampler run pass by pass, return_sequence=True, keeps the fused
 * run's draws); the x_T draw is taken only when x_T is NULL. */
int fd_sample_coefs(const fd_model* m, const float* mel, const float* ce, const float* den,
                    const float* sg, const float* steps, int N, const float* x_T,
                    const float* noise, unsigned long long seed, const int* utt_ids, const int* lens,
                    int draw0, float* wav, int B, int Tc, void* workspace, size_t ws_bytes, void* stream);

/* The sampler's x_T ~ N(0,1) draw alone (util.py:208): exactly the [B,L] array fd_sample /
 * fd_sample_coefs draw when their x_T is NULL (same seed and utt_ids), written to x_T.  A
 * pass-by-pass run (return_sequence=True) takes its first state from here. */
int fd_draw_x_T(const fd_model* m, float* x_T, int B, int Tc, unsigned long long seed, const int* utt_ids,
                void* stream);

/* ==================================================================== NSF-HiFiGAN
 * SVS vocoder -- replaces modules/nsf_hifigan/models.py:222-283
 * (Generator, with SourceModuleHnNSF/SineGen :100-219 and ResBlock1/2 :36-97) as
 * called by NsfHifiGAN.spec2wav_torch (component/vocoder/nsf_hifigan.py:29-56).
 */
typedef struct nsf_model nsf_model;

typedef struct {
  int num_mels;                    /* 128 (handler/base_config.yaml:7) */
  int upsample_initial_channel;    /* 512 */
  int num_upsamples;               /* len(upsample_rates) <= 6 */
  int upsample_rates[6];           /* 8, 8, 2, 2 (hop 512) */
  int upsample_kernel_sizes[6];    /* 16, 16, 4, 4; k % u == 0, k - u even */
  int resblock;                    /* 1 (ResBlock1) or 2 (ResBlock2) */
  int num_kernels;                 /* len(resblock_kernel_sizes) <= 4 */
  int resblock_kernel_sizes[4];    /* 3, 7, 11 (odd, <= 11) */
  int num_dilations;               /* len(resblock_dilation_sizes[j]) <= 4 */
  int resblock_dilation_sizes[4][4];
  int sampling_rate;               /* 44100 */
  int harmonic_num;                /* 8 (models.py:229) */
} nsf_dims;

/* Parameter order = the reference state dict after remove_weight_norm (models.py:285-293):
 *   m_source.l_linear.{weight,bias}, noise_convs.i.{weight,bias} (i < num_upsamples),
 *   conv_pre.{weight,bias}, ups.i.{weight [Cin,Cout,k], bias},
 *   resblocks.n.convs1.j / convs2.j (ResBlock1) or convs.j (ResBlock2) {weight,bias},
 *   conv_post.{weight,bias}.  All device pointers, fp32. */
int nsf_num_params(const nsf_dims* dims);
/* dtype PD_DTYPE_F32: exact fp32 (parity path); PD_DTYPE_BF16: bf16 weights/activations on the
 * MFMA, fp32 accumulate, fp32 source module and epilogues. */
int nsf_create(const nsf_dims* dims, const float* const* params, int dtype, void* stream, nsf_model** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void nsf_destroy(nsf_model* m);
int nsf_hop(const nsf_model* m);   /* prod(upsample_rates) */
size_t nsf_workspace_size(const nsf_model* m, int B, int T);
/* NSF_OPT_SMALL_MAX: ResBlock convs with at most this many channels run on the LDS/VALU small-channel
 * kernel (default 16, measured; 0 = never).  Set before the first forward call. */
#define NSF_OPT_SMALL_MAX 0
/* NSF_OPT_WCONV: 1 (default) runs the bf16 ResBlock convs with 16..256 channels on the windowed
 * MFMA conv kernels (input window staged once in LDS for all taps), ahead of
 * NSF_OPT_SMALL_MAX; 0 = the implicit-GEMM engine / small kernel.  No effect on the fp32 path. */
#define NSF_OPT_WCONV 1
/* NSF_OPT_PAIR: 1 (default) runs each ResBlock1 conv pair c2(lrelu(c1(lrelu(x)))) + x with 32, 64 or 128
 * channels (16: NSF_OPT_PAIR16) as ONE windowed launch (the inner activation stays in LDS, x is read once); 0 = two
 * windowed launches with the inner activation through HBM in bf16.  Same roundings either way. */
#define NSF_OPT_PAIR 2
/* NSF_OPT_PAIR16: 1 (default) runs the 16-channel ResBlock1 pairs of the shipped shapes (taps 3/7/11,
 * dilation 1/3/5) the same way, on 16x16x32 MFMAs; 0 = two launches for them.  Needs NSF_OPT_PAIR. */
#define NSF_OPT_PAIR16 3
/* NSF_OPT_UPS_NC: 1 (default) lets the bf16 windowed upsample compute the noise conv of its stage itself when
 * the source kernel has at most 8 taps (the last three stages) instead of reading nsf_noise_conv's output;
 * 0 = always the separate noise conv.  Same fp32 operations in the same order. */
#define NSF_OPT_UPS_NC 4
/* NSF_OPT_RB16 (r06): 1 (default) runs each 16-channel ResBlock1 of the shipped shapes (taps 3/7/11, c1
 * dilations 1, 3, 5) as ONE launch that keeps the residual in registers across its three conv pairs and reads
 * x / writes the ResBlock sum once (32-tile windows, 4 waves); 2 = 64-tile windows of 8 waves; 0 = one
 * launch per pair (NSF_OPT_PAIR16).  Same roundings and MFMA order: bit-identical either way. */
#define NSF_OPT_RB16 5
/* NSF_OPT_RB32 / NSF_OPT_RB64 (r06): the same whole-ResBlock1 launch at 32 / 64 channels, for the kernel sizes
 * whose bit is set (1: taps 3, 2: taps 7, 4: taps 11); 0 = one launch per pair.  Bit-identical either way.
 * Defaults: RB32 1 (taps 3 only), RB64 0 (measured). */
#define NSF_OPT_RB32 6
#define NSF_OPT_RB64 7
/* NSF_OPT_C256 (r06): the 256-channel ResBlock convs' block shape -- 0: 4 waves and 128 output channels per
 * block (two blocks stage each row tile's window), 1 (default): 8 waves and all 256.  Bit-identical. */
#define NSF_OPT_C256 8
/* NSF_OPT_NC_MFMA (r06): 2 (default) runs the first two stages' source convs (K = 128 / 16, stride K / 2) on the
 * f32 MFMA (fmaf chains from the bias, k ascending: bit-identical), 1 only the K = 128 one, 0 = the fp32 VALU kernel. */
#define NSF_OPT_NC_MFMA 9
int nsf_set_option(nsf_model* m, int option, int value);

/* spec2wav_torch(mel, f0=f0) for a batch of independent utterances:
 *   mel [B,T,num_mels] time-major, scaled by mel_scale on load: 2.30259 turns the log10
 *   mel of spec2wav_torch into the natural-log mel the Generator takes (nsf_hifigan.py:50-53);
 *   1.0 is Generator.forward(c, f0) itself (models.py:265)
 *   f0  [B,T] Hz (0 = unvoiced)
 *   rand_ini [harmonic_num+1] (torch.rand(1,dim), models.py:139; element 0 ignored) and
 *   noise [B, T*hop, harmonic_num+1] (randn_like, models.py:182), or NULL -> Philox from seed
 *   wav [B, T*hop] output in [-1, 1]. */
int nsf_forward(const nsf_model* m, const float* mel, float mel_scale, const float* f0, const float* rand_ini,
                const float* noise, unsigned long long seed, const int* utt_ids, const int* lens, float* wav,
                int B, int T, void* workspace, size_t ws_bytes, void* stream);

/* ============================================================ condition encoder
 * SVS teacher condition -- replaces ProDiffTeacher.forward_condition
 * (modules/svs/prodiff_teacher.py:103-146): FastspeechEncoder (modules/fastspeech/
 * tts_modules.py:232-330: token + position embedding, enc_layers x EncSALayer with 2-head
 * self-attention and the k=9 conv FFN, final LayerNorm), mel2ph_to_dur (:223-229), the
 * mel2ph length-regulator gather and the pitch / speaker / gender / voicing / breath sums.
 */
typedef struct pd_cond pd_cond;

typedef struct {
  int vocab_size;            /* len(ph_encoder)                         prodiff_teacher.py:13 */
  int hidden_size;           /* H: 256 (handler/base_config.yaml:112), multiple of 64       */
  int enc_layers;            /* 4                                                            */
  int enc_ffn_kernel_size;   /* 9 (odd, <= 11)                                               */
  int num_heads;             /* 2; head dim H / num_heads in {64, 128, 256}                  */
  int num_spk;               /* spk_embed rows                                               */
  int num_langs;             /* lang_embed rows = len(hparams["languages"]) + 1              */
  int use_dur_embed, use_spk_id, use_gender_id, use_lang_id, use_voicing_embed, use_breath_embed;
  int rel_pos;               /* > 0: RelPositionalEncoding (tts_modules.py:299-300,324-325,
                                espnet_positional_embedding.py:89-115) instead of the sinusoid,
                                with a table of max(rel_pos, 5000) rows (< 0 rejected): the
                                reference's table starts at 5000 rows and extend_pe (:24-45)
                                keeps the longest input's length, which then sets the
                                reversed positions of every later, shorter batch         */
} pd_cond_dims;

/* Parameter order = the reference state-dict order (buffers and `diffusion.*` skipped), fp32:
 *   for l < enc_layers: encoder.layers.l.op.{layer_norm1.weight, layer_norm1.bias,
 *       self_attn.in_proj_weight [3H,H], self_attn.out_proj.weight [H,H], layer_norm2.weight,
 *       layer_norm2.bias, ffn.ffn_1.weight [4H,H,k], ffn.ffn_1.bias, ffn.ffn_2.weight [H,4H],
 *       ffn.ffn_2.bias},
 *   encoder.layer_norm.{weight,bias}, encoder.embed_tokens.weight [V,H],
 *   [dur_embed.{weight [H,1],bias}], [spk_embed.weight], [gender_embed.weight [2,H]],
 *   [lang_embed.weight], pitch_embed.{weight,bias}, [voicing_embed.{weight,bias}],
 *   [breath_embed.{weight,bias}]   ([...] present iff its use_* flag is set).
 * The reference's add_gender_embed looks gender ids up in lang_embed (prodiff_teacher.py:95);
 * that is reproduced, so use_gender_id requires use_lang_id. */
int pd_cond_num_params(const pd_cond_dims* dims);
int pd_cond_create(const pd_cond_dims* dims, const float* const* params, int dtype, void* stream,
                   pd_cond** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_cond_destroy(pd_cond* h);
size_t pd_cond_workspace_size(const pd_cond* h, int B, int T_txt, int T_mel);

/* forward_condition's inputs, all device pointers (int64 = torch.long), NULL when absent:
 *   txt_tokens [B,T_txt] (0 = padding), mel2ph [B,T_mel] (0 = padding frame, else token
 *   index + 1, <= T_txt), f0 [B,T_mel] Hz, lang_seq [B,T_txt], spk_embed_id [B] or
 *   spk_mix_embed [B, spk_mix_frames (1 or T_mel), H], gender_embed_id [B] or
 *   gender_mix_embed [B, gender_mix_frames, H], voicing [B,T_mel], breath [B,T_mel].
 * Embedding ids outside their table (an IndexError in the reference) are clamped on the device
 * and mel2ph values above T_txt give zero frames, so a malformed input cannot fault the GPU. */
typedef struct {
  const long long* txt_tokens;
  const long long* mel2ph;
  const float* f0;
  const long long* lang_seq;
  const long long* spk_embed_id;
  const float* spk_mix_embed;
  int spk_mix_frames;
  const long long* gender_embed_id;
  const float* gender_mix_embed;
  int gender_mix_frames;
  const float* voicing;
  const float* breath;
  /* Ragged token batch (device, B ints, or NULL = every row T_txt tokens): row b's phonemes are its
   * first txt_lens[b] tokens.  The FFN conv (k = 9 over tokens) then reads zero past each row's own
   * end -- the zero padding of the row encoded alone (B = 1, T_txt = txt_lens[b]), the reference's
   * one-segment-at-a-time inference -- where it would otherwise read the padded rows' LayerNorm(0) =
   * beta (common_layers.py:668-669).  Attention and LayerNorm already mask padding tokens. */
  const int* txt_lens;
} pd_cond_inputs;

/* cond [B,T_mel,H] time-major (what pd_prodiff_sample / pd_reflow_sample take), and optionally
 * enc_out [B,T_txt,H] = the FastspeechEncoder output (tts_modules.py:310-317); either may be
 * NULL (not both); with cond NULL, mel2ph / T_mel still feed the duration embedding.  Every
 * utterance needs at least one non-padding token. */
int pd_cond_forward(const pd_cond* h, const pd_cond_inputs* in, float* cond, float* enc_out, int B,
                    int T_txt, int T_mel, void* workspace, size_t ws_bytes, void* stream);

/* ============================================================ variance predictors
 * The encoders of the pitch and duration predictors, the two models that run before the teacher
 * when a segment carries no f0 / phoneme durations (handler/infer/handler.py:218-234,262-278).
 * Both are built on the FFT-block stack of the condition encoder (same kernels, their own widths).
 *
 * pd_pitch_cond -- everything of PitchPredictor.forward (modules/variance_predictor/
 * pitch_predictor.py:57-121) that builds the rectified-flow sampler's `cond`: the phoneme
 * FastspeechEncoder, the NoteEncoder (tts_modules.py:332-365), note_encode_out_linear, the two
 * length-regulator gathers and the speaker / retake / delta-pitch embeddings.  The sampler itself is
 * pd_reflow_sample over the predictor's WaveNet.
 */
typedef struct pd_pitch_cond pd_pitch_cond;

typedef struct {
  int vocab_size;             /* len(ph_encoder); embed_tokens has vocab_size + 1 rows (pitch_predictor.py:14) */
  int hidden_size;            /* H: 256, multiple of 64                                                        */
  int enc_layers;             /* 4                                                                             */
  int enc_ffn_kernel_size;    /* 9 (odd, <= 11)                                                                */
  int num_heads;              /* 2; head dim in {64, 128, 256}                                                 */
  int note_hidden_size;       /* Hn: 128 (handler/base_config.yaml:141-145), multiple of 64                    */
  int note_layers;            /* 4                                                                             */
  int note_ffn_kernel_size;   /* 9                                                                             */
  int note_heads;             /* 2                                                                             */
  int num_spk;                /* spk_embed rows = len(hparams['datasets'])                                     */
  int use_spk_id;
} pd_pitch_cond_dims;

/* Parameter order = the reference state-dict order (buffers and `diffusion.*` skipped), fp32:
 *   encoder.layers.l.op.* (the ten of pd_cond) for l < enc_layers, encoder.layer_norm.{weight,bias},
 *   encoder.embed_tokens.weight [V+1,H], dur_embed.{weight [H,1],bias},
 *   note_encoder.layers.l.op.* for l < note_layers, note_encoder.layer_norm.{weight,bias},
 *   note_encoder.note_midi_embed.{weight [Hn,1],bias}, note_encoder.note_dur_embed.{weight [Hn,1],bias},
 *   note_encode_out_linear.{weight [H,Hn],bias}, [spk_embed.weight [num_spk,H]],
 *   delta_pitch_embed.{weight [H,1],bias}, pitch_retake_embed.weight [2,H]. */
int pd_pitch_cond_num_params(const pd_pitch_cond_dims* dims);
int pd_pitch_cond_create(const pd_pitch_cond_dims* dims, const float* const* params, int dtype, void* stream,
                         pd_pitch_cond** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_pitch_cond_destroy(pd_pitch_cond* h);
size_t pd_pitch_cond_workspace_size(const pd_pitch_cond* h, int B, int T_txt, int T_note, int T_mel);

/* PitchPredictor.forward's inputs, device pointers, NULL when absent:
 *   txt_tokens [B,T_txt] int64 (0 = padding), mel2ph [B,T_mel] int64 (0 = padding frame, else token + 1),
 *   note_midi [B,T_note] float (< 0 = padding note), note_rest [B,T_note] bytes (torch.bool),
 *   mel2note [B,T_mel] int64 (0 = padding frame, else note + 1), spk_id [B] int64 (required with
 *   use_spk_id), pitch_expr [B] float, pitch / base_pitch [B,T_mel] float and pitch_retake [B,T_mel]
 *   bytes (torch.bool).  With r = pitch_retake (1 everywhere when it is NULL):
 *     retake = pitch_expr ? E[1] e + E[0] (1 - e), e = pitch_expr[b] r   :   E[r]       (E = pitch_retake_embed)
 *     delta  = pitch_retake ? (pitch - base_pitch) [!r] : 0             (pitch and base_pitch then required)
 *   txt_lens / note_lens: ragged batches (B ints each, or NULL) as pd_cond_inputs.txt_lens -- every row then
 *   equals the segment encoded alone.
 * Ids outside their tables are clamped; mel2ph / mel2note values outside [1, T_txt] / [1, T_note] gather a zero
 * row: a malformed input cannot fault the GPU. */
typedef struct {
  const long long* txt_tokens;
  const long long* mel2ph;
  const float* note_midi;
  const unsigned char* note_rest;
  const long long* mel2note;
  const long long* spk_id;
  const float* pitch_expr;
  const float* pitch;
  const float* base_pitch;
  const unsigned char* pitch_retake;
  const int* txt_lens;
  const int* note_lens;
} pd_pitch_cond_inputs;

/* cond [B,T_mel,H] time-major (what pd_reflow_sample takes):
 *   cond[f] = pad0(enc)[mel2ph[f]] + pad0(note_lin)[mel2note[f]] + spk + retake + (delta w + b)
 * with no final mel2ph > 0 mask (the reference has none: padding frames keep spk + retake + delta). */
int pd_pitch_cond_forward(const pd_pitch_cond* h, const pd_pitch_cond_inputs* in, float* cond, int B, int T_txt,
                          int T_note, int T_mel, void* workspace, size_t ws_bytes, void* stream);

/* pd_dur -- DurPredictor.forward (modules/variance_predictor/dur_predictor.py:31-36): the
 * FastspeechEncoder with extra_embed = onset_embed(onset) + word_dur_embed(word_dur), then
 * DurationPredictor (tts_modules.py:59-132): n_layers x (k-tap conv, ReLU, LayerNorm eps 1e-12,
 * padding mask), a Linear to one value per token, the mask again, and out2dur. */
typedef struct pd_dur pd_dur;

typedef struct {
  int vocab_size;
  int hidden_size, enc_layers, enc_ffn_kernel_size, num_heads;   /* as pd_cond_dims */
  int n_layers;               /* 5   (handler/base_config.yaml:120-126) */
  int n_chans;                /* 512, multiple of 32                     */
  int kernel_size;            /* 3 (odd, <= 11)                          */
  float log_offset;           /* 1.0                                     */
} pd_dur_dims;

/* Parameter order = the reference state-dict order: the encoder's (as above, embed_tokens [V,H]),
 * onset_embed.weight [2,H], word_dur_embed.{weight [H,1],bias}, for i < n_layers:
 * dur_pred.conv.i.1.{weight [C,Cin,k],bias}, dur_pred.conv.i.3.{weight,bias}, then
 * dur_pred.linear.{weight [1,C],bias}. */
int pd_dur_num_params(const pd_dur_dims* dims);
int pd_dur_create(const pd_dur_dims* dims, const float* const* params, int dtype, void* stream, pd_dur** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_dur_destroy(pd_dur* h);
size_t pd_dur_workspace_size(const pd_dur* h, int B, int T_txt);

/* txt_tokens [B,T_txt] int64 (0 = padding), onset [B,T_txt] int64 in {0,1} (clamped), word_dur [B,T_txt]
 * float, txt_lens as pd_cond_inputs.txt_lens. */
typedef struct {
  const long long* txt_tokens;
  const long long* onset;
  const float* word_dur;
  const int* txt_lens;
} pd_dur_inputs;

/* log_out [B,T_txt]: the log-domain prediction (linear output times the padding mask, tts_modules.py:126-127);
 * dur_out [B,T_txt]: max(exp(log_out) - log_offset, 0), DurationPredictor.forward(infer=True).  Either may be
 * NULL, not both. */
int pd_dur_forward(const pd_dur* h, const pd_dur_inputs* in, float* log_out, float* dur_out, int B, int T_txt,
                   void* workspace, size_t ws_bytes, void* stream);

/* ================================================================ mel analysis
 * pd_mel -- STFT.get_mel (modules/nsf_hifigan/nvSTFT.py:48-98), the analysis half of the vocoder contract
 * (component/vocoder/nsf_hifigan.py:93-110 wav2spec): reflect padding, a center=False STFT with a periodic
 * Hann window, the magnitude, the key-shift rescaling of the bins, the mel filterbank and
 * log(clamp(., clip_val)), in one kernel.  fp32 only.  With
 *   f = 2^(keyshift/12), nf = round(n_fft f), wn = round(win_size f), hn = round(hop_size speed)
 * (round half to even, as numpy) a signal of L samples is padded by (wn - hn)/2 on the left and
 * (wn - hn + 1)/2 on the right and gives T = 1 + (L + wn - hn - nf) / hn frames; frame t covers the padded
 * samples [t hn, t hn + nf), the window sits centred in it.  Of the n_fft/2 + 1 output bins the first
 * nb = min(n_fft/2, nf/2) + 1 are DFT bins of the nf-point frame (times win_size / wn when keyshift != 0),
 * the rest are zero.  center=True is not offered.  A handle serves one (keyshift, speed). */
typedef struct pd_mel pd_mel;

typedef struct {
  int n_fft;       /* 2048 (SVS), 1024; <= 65536                                        */
  int win_size;    /* <= n_fft                                                          */
  int hop_size;
  int n_mels;      /* <= 128                                                            */
  float keyshift;  /* semitones, 0 = none                                               */
  float speed;     /* 1 = none                                                          */
  float clip_val;  /* 1e-5, > 0                                                         */
} pd_mel_dims;

/* mel_basis: device, [n_mels][n_fft/2 + 1] row-major (librosa.filters.mel's layout), read on `stream`.
 * Builds the two windowed DFT tables on the device (double precision, phase reduced as the integer
 * (n k) mod nf, rounded once to f32) into the handle's weight pool.  Dimensions whose 31 hops + one
 * frame exceed the 160 KiB LDS, or n_mels > 128, return PD_ERR_UNSUPPORTED. */
int pd_mel_create(const pd_mel_dims* dims, const float* mel_basis, void* stream, pd_mel** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_mel_destroy(pd_mel* h);
/* T for a signal of n_samples; 0 below pd_mel_min_samples. */
int pd_mel_frames(const pd_mel* h, int n_samples);
/* The shortest legal signal: the larger pad + 1 (reflect padding needs L > pad), and at least one
 * whole frame (nf - wn + hn, which only exceeds the former when win_size < n_fft). */
int pd_mel_min_samples(const pd_mel* h);
/* 0: the kernel needs no scratch (`workspace` may be NULL). */
size_t pd_mel_workspace_size(const pd_mel* h, int B, int L);
/* wav [B][L] -> out [B][T][n_mels] time-major = out_scale * log(max(mel, clip_val)), T = pd_mel_frames(h, L);
 * spec_out [B][T][n_fft/2 + 1] (the magnitude spectrum) or NULL.  lens: int32 [B] samples per row or NULL;
 * row b then equals the signal of lens[b] samples analysed alone, its frames past pd_mel_frames(h, lens[b])
 * are unspecified; a lens[b] outside [pd_mel_min_samples, L] is clamped into it (that row's output is
 * unspecified, every access stays inside the row).  A frame's values do not depend on its batch row, on B
 * or on where it falls in a block.  L < pd_mel_min_samples returns PD_ERR_ARG. */
int pd_mel_forward(const pd_mel* h, const float* wav, const int* lens, float out_scale, float* out, float* spec_out,
                   int B, int L, void* workspace, size_t ws_bytes, void* stream);

/* ================================================================ sample-rate conversion
 * pd_resample -- the polyphase windowed-sinc resampler that torchaudio.functional.resample defines, which the
 * reference reaches as torchaudio.transforms.Resample(sr, 16000, lowpass_filter_width=128) in front of the
 * RMVPE pitch extractor (component/pe/rmvpe.py:49); its other two resamplers, librosa.load(sr=) in wav2spec
 * (component/vocoder/nsf_hifigan.py:96) and librosa.resample(..., 'kaiser_best') (utils/data_gen_utils.py:51),
 * are soxr / resampy filters that this one replaces but does not reproduce sample for sample.  fp32 only.  With
 *   g = gcd(orig_freq, new_freq), o = orig_freq / g, n = new_freq / g, base = min(o, n) rolloff,
 *   W = ceil(lowpass_filter_width o / base), K = 2 W + o,
 *   t = clamp(((k - W) / o - p / n) base, -lowpass_filter_width, lowpass_filter_width),
 *   h[p][k] = sinc(t) w(t) base / o,   w = cos(pi t / (2 width))^2 (hann), I0(beta sqrt(1 - (t / width)^2)) / I0(beta) (kaiser)
 * (float64, rounded once to f32) a row of L samples gives ceil(n L / o) outputs
 *   y[q n + p] = sum_{k < K} h[p][k] x[q o + k - W],   x zero outside [0, L),
 * each one f32 fmaf chain from zero over k ascending. */
typedef struct pd_resample pd_resample;

#define PD_RESAMPLE_HANN 0    /* sinc_interp_hann   */
#define PD_RESAMPLE_KAISER 1  /* sinc_interp_kaiser */

typedef struct {
  int orig_freq, new_freq;   /* Hz, > 0 (only their ratio matters)                         */
  int lowpass_filter_width;  /* zero crossings of the sinc kept on each side: 6, 64, 128   */
  double rolloff;            /* 0.99: cutoff as a fraction of the lower Nyquist frequency  */
  int method;                /* PD_RESAMPLE_HANN / PD_RESAMPLE_KAISER                      */
  double beta;               /* Kaiser only, in [0, 256]: 14.769656459379492               */
} pd_resample_dims;

/* Builds the table on the device (double precision, one rounding) into the handle's weight pool, stream-ordered.
 * Null or non-positive arguments return PD_ERR_ARG before anything is allocated.  A block keeps the samples of
 * 32 output frames and their 32 n outputs in LDS: a pair with 32 (o + n) + 4 W floats beyond the 160 KiB LDS
 * (or a table beyond 64 MiB) returns PD_ERR_UNSUPPORTED.  Every pair of common audio rates (8 to 192 kHz, o and
 * n <= 640) fits at the widths above. */
int pd_resample_create(const pd_resample_dims* dims, void* stream, pd_resample** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_resample_destroy(pd_resample* h);
/* ceil(n n_samples / o), in 64-bit integers; 0 for a null handle or n_samples <= 0. */
size_t pd_resample_out_samples(const pd_resample* h, int n_samples);
/* The reduced rates and the half width W (K = 2 W + o taps per phase); any pointer may be NULL. */
int pd_resample_taps(const pd_resample* h, int* o, int* n, int* W);
/* table_out: device f32 [n][K], the table h as the kernel uses it, written on `stream`. */
int pd_resample_kernel(const pd_resample* h, float* table_out, void* stream);
/* 0: the kernel needs no scratch (`workspace` may be NULL). */
size_t pd_resample_workspace_size(const pd_resample* h, int B, int L);
/* wav [B][L] -> out [B][pd_resample_out_samples(h, L)].  lens: int32 [B] samples per row or NULL; row b then
 * equals its first lens[b] samples resampled alone, its outputs past pd_resample_out_samples(h, lens[b]) are
 * unspecified (not written); a lens[b] outside [0, L] is clamped into it.  An output's value does not depend on
 * its batch row, on B or on where its frame falls in a block.  Samples must be finite (the table's zero padding
 * multiplies neighbouring samples).  One launch, stream-ordered, no allocation. */
int pd_resample_forward(const pd_resample* h, const float* wav, const int* lens, float* out, int B, int L,
                        void* workspace, size_t ws_bytes, void* stream);

/* ================================================================ pitch extraction
 * pd_mel_create_centered -- a second constructor of pd_mel with the framing of torch.stft(center=True), which
 * the RMVPE front end uses (modules/rmvpe/spec.py:48-56): reflect padding of nf/2 samples on both sides,
 * T = 1 + L / hn frames, frame t centred on sample t hn.  Everything else (window, key shift, bins, basis, log)
 * is as pd_mel_create; pd_mel_frames and pd_mel_min_samples (nf/2 + 1) follow the handle's framing. */
int pd_mel_create_centered(const pd_mel_dims* dims, const float* mel_basis, void* stream, pd_mel** out);

/* pd_rmvpe -- E2E0 (modules/rmvpe/model.py:8-32): the log-mel as a one-channel image [B,1,T,F] through
 * encoder.bn (eval BatchNorm on the input, applied to the in-range pixels only: the first conv's zero padding
 * comes after it), en_de_layers encoder levels of n_blocks ConvBlockRes at en_out_channels * 2^i channels, each
 * followed by AvgPool2d(2,2) (the unpooled output is the level's skip), inter_layers * n_blocks ConvBlockRes at
 * the bottom, en_de_layers decoder levels (ConvTranspose2d 3x3 stride 2 padding 1 output_padding 1 without
 * bias + BN + ReLU, cat with the skip, n_blocks ConvBlockRes), cnn = Conv2d(en_out_channels, 3, 3x3) with bias,
 * feat[b][t][c * n_mels + f], then a bidirectional one-layer GRU (gate order r, z, n; h_0 = 0) and
 * Linear + Sigmoid, or with n_gru = 0 Linear + Sigmoid on feat (deepunet.py, seq.py).
 *   ConvBlockRes(x) = ReLU(BN(conv3x3(ReLU(BN(conv3x3(x)))))) + s(x), s = identity, or a 1x1 conv with bias
 * when the channel count changes.  Every BatchNorm is the eval form (eps 1e-5); create folds each post-conv one
 * into its conv in double precision (w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps)), rounded
 * once.  fp32 by default; pd_rmvpe_set_option below moves the 3x3 convs' operands and the recurrent product to bf16. */
typedef struct pd_rmvpe pd_rmvpe;

typedef struct {
  int n_blocks;         /* 4; 1..16                                                        */
  int n_gru;            /* 1; 0 (Linear head on feat) or 1                                 */
  int en_de_layers;     /* 5; 1..5, n_mels a multiple of 2^en_de_layers                    */
  int inter_layers;     /* 4; 1..16                                                        */
  int en_out_channels;  /* 16; a multiple of 16, <= 256                                    */
  int n_mels;           /* 128; 3 n_mels a multiple of 32                                  */
  int n_class;          /* 360                                                             */
  int gru_hidden;       /* 256 (the only size the recurrence kernel is built for)          */
} pd_rmvpe_dims;

/* Parameter order = the reference state-dict order without any num_batches_tracked and without unet.tf.* (the
 * TimbreFilter is built but never called).  With bn(p) = p.{weight,bias,running_mean,running_var} and
 * block(p) = p.conv.0.weight [Co,Ci,3,3], bn(p.conv.1), p.conv.3.weight [Co,Co,3,3], bn(p.conv.4), and where
 * Ci != Co p.shortcut.{weight [Co,Ci,1,1],bias}:
 *   bn(unet.encoder.bn);
 *   for i < en_de_layers, j < n_blocks: block(unet.encoder.layers.i.conv.j)       (Ci = 1 for i = j = 0);
 *   for i < inter_layers, j < n_blocks: block(unet.intermediate.layers.i.conv.j);
 *   for i < en_de_layers: unet.decoder.layers.i.conv1.0.weight [Ci,Co,3,3], bn(unet.decoder.layers.i.conv1.1),
 *       for j < n_blocks: block(unet.decoder.layers.i.conv2.j)                    (Ci = 2 Co for j = 0);
 *   cnn.{weight [3,C,3,3],bias};
 *   n_gru = 1: fc.0.gru.{weight_ih_l0 [768,3 n_mels],weight_hh_l0 [768,256],bias_ih_l0,bias_hh_l0}, the same four
 *       with the suffix _reverse, fc.1.{weight [n_class,512],bias};  n_gru = 0: fc.0.{weight [n_class,3 n_mels],bias}.
 * 0 for dimensions outside the supported set. */
int pd_rmvpe_num_params(const pd_rmvpe_dims* dims);
/* Folds and packs every parameter into the handle's weight pool on `stream` (the caller's tensors are not read
 * after the stream has passed the call).  A dtype other than PD_DTYPE_F32, or dimensions outside the ranges
 * above, return PD_ERR_UNSUPPORTED before anything is allocated. */
int pd_rmvpe_create(const pd_rmvpe_dims* dims, const float* const* params, int dtype, void* stream, pd_rmvpe** out);
/* The caller must ensure that no call on the handle is still in flight (synchronize its streams first). */
void pd_rmvpe_destroy(pd_rmvpe* h);
/* Two options of the handle, each PD_DTYPE_F32 (the default) or PD_DTYPE_BF16; pd_rmvpe_create itself takes
 * PD_DTYPE_F32 only.
 *   PD_RMVPE_OPT_CONV_DTYPE  bf16: every 3x3 conv with C_in a multiple of 16 (all but the first conv and `cnn`), its
 *       1x1-shortcut accumulator, the transposed convs and the two-source cat form run on v_mfma_f32_32x32x16_bf16.
 *       The input values are rounded once to bf16 (nearest even) after the in-image select, so border and stuffed
 *       zeros stay zeros, and meet the bf16 copy of the folded weights (the f32 folded value as create rounds it,
 *       rounded once more).  Accumulation, folded bias, ReLU, residual add and every stored map stay fp32.
 *   PD_RMVPE_OPT_GRU_DTYPE   bf16: the recurrent product is bf16(h_{t-1}) bf16(W_hh)^T on v_mfma_f32_16x16x32_bf16,
 *       summed in f32; b_hh, the gates and the blend h = (1 - z) n + z h_{t-1} use the unrounded fp32 h_{t-1}; the
 *       output and the carried state are fp32.  Without a GRU (n_gru = 0) the option is accepted and has no effect.
 * The first conv, `cnn`, the pools, the W_ih projection, the head and the sigmoid are fp32 in every mode.  The first
 * switch of either option to bf16 allocates the bf16 mirror of the weight pool and fills it on `stream`
 * (pd_live_device_bytes counts it, pd_rmvpe_destroy returns it); later switches only flip the mode and touch
 * nothing.  Workspace sizes do not change.  With both options at PD_DTYPE_F32 every kernel launched is the one
 * launched without this call.  The bit-exact promises of pd_rmvpe_forward and pd_rmvpe_forward_ragged (rows,
 * batch position, ragged rows against their single runs) hold within one mode.  The caller must ensure that no
 * call on the handle is in flight.  A null handle, an unknown option or any other value: PD_ERR_ARG, nothing changes. */
#define PD_RMVPE_OPT_CONV_DTYPE 0
#define PD_RMVPE_OPT_GRU_DTYPE 1
int pd_rmvpe_set_option(pd_rmvpe* h, int option, int value, void* stream);
size_t pd_rmvpe_workspace_size(const pd_rmvpe* h, int B, int T);
/* mel [B][T][n_mels] time-major natural-log mel (what pd_mel_forward writes) -> hidden [B][T][n_class], the
 * salience in [0, 1]; feat [B][T][3 n_mels] (the cnn output, feature index c n_mels + f) or NULL.  T must be a
 * positive multiple of 2^en_de_layers (PD_ERR_ARG otherwise; the caller pads with the value 0.0 as
 * component/pe/rmvpe.py:29-33 does, those frames are network input).  All rows share T.  Stream-ordered, no
 * allocation, no synchronisation, capturable.  An output row depends neither on B nor on its batch position. */
int pd_rmvpe_forward(const pd_rmvpe* h, const float* mel, float* hidden, float* feat, int B, int T, void* workspace,
                     size_t ws_bytes, void* stream);
/* pd_rmvpe_forward for a ragged batch.  frames: device int32 [B], row b's real mel frames T_b in [1, T]; T stays a
 * positive multiple of 2^en_de_layers and sizes the tensors and the workspace exactly as above.  Row b is
 * computed as the image of n_b = T_b rounded up to 2^en_de_layers rows: its input frames in [T_b, n_b) read as
 * the value 0.0 (network input, as the caller's padding above), whatever mel holds there or past n_b is never
 * used (it may be NaN), and at level l every pixel with y >= n_b >> l lies outside the image, for every conv
 * and for the recurrence, whose reverse direction starts at frame n_b - 1 from h = 0.  hidden[b][t] and
 * feat[b][t] for t < T_b equal, bit for bit, pd_rmvpe_forward of that row alone with T = n_b; for t >= T_b they
 * are unspecified.  A frames[b] outside [1, T] is clamped into it (that row's output is unspecified, every
 * access stays inside the row).  frames == NULL returns PD_ERR_ARG.  Same launches as pd_rmvpe_forward (conv
 * tiles that lie past their row's height return at once); stream-ordered, no allocation, no synchronisation,
 * capturable. */
int pd_rmvpe_forward_ragged(const pd_rmvpe* h, const float* mel, const int* frames, float* hidden, float* feat, int B,
                            int T, void* workspace, size_t ws_bytes, void* stream);
/* to_local_average_f0 (modules/rmvpe/utils.py:8-23): hidden [B][T][n_class] -> f0 [B][T] in Hz.  c = the first
 * index of the row maximum, or center[b][t] (int64 [B][T], device) when center is non-NULL, clamped into
 * [0, n_class); over i in [max(c - 4, 0), min(c + 5, n_class)): cents = sum h_i (20 i + cents_const) /
 * (sum h_i + [sum h_i == 0]), f0 = 10 * 2^(cents / 1200), and f0 = 0 where the row maximum is < thred.  The sums
 * run in double precision; cents_const is the reference's CONST = 1997.3794084376191, passed as a double so that
 * it is not rounded to f32 on the way. */
int pd_rmvpe_decode(const float* hidden, float* f0, int B, int T, int n_class, float thred, const long long* center,
                    double cents_const, void* stream);

/* to_viterbi_f0's path (modules/rmvpe/utils.py:26-43: librosa.sequence.viterbi over the salience with a banded
 * transition) for each row of hidden [B][T][n_class] (float32 >= 0).  In double throughout:
 *   p[t][j] = h[t][j] / sum_j h[t][j]  (a frame whose sum is not positive counts as uniform, p = 1 / n_class; the
 *   reference yields NaN there),  lp = log(p + tiny), tiny = FLT_MIN;
 *   val[0][j] = lp[0][j] + log_init;  val[t][j] = lp[t][j] + max_i (val[t-1][i] + lt[i][j]),  ptr[t][j] = the lowest
 *   i attaining the max;  path[T-1] = the lowest argmax_j val[T-1][j],  path[t] = ptr[t+1][path[t+1]];
 *   logp[b] = val[T-1][path[T-1]] (librosa's return_logp), or logp = NULL.
 * lt[i][j] = log_band[i][j - i + width - 1] for |i - j| < width and log_off outside the band; log_off must lie
 * below every in-band entry by more than the spread of val that one frame's lp can make up (the caller's tables,
 * log(A + tiny) of A[i][j] = max(width - |i - j|, 0) row-normalised, do: the band holds values >= -6.9, log_off is
 * -87.3): the kernel evaluates the band and one out-of-band candidate, the lowest global argmax of val[t-1], which
 * under that condition equals the dense maximum and its lowest argmax exactly.  The reference normalises p in
 * float32; this entry point does it in double.
 * n_class <= 512 and width <= 64 (PD_ERR_UNSUPPORTED beyond; widths above 30 read the band from memory instead of
 * registers).  Back pointers are resolved in chunks of PD_RMVPE_VITERBI_CHUNK frames (pd_rmvpe_viterbi_chunk
 * returns the library's value).  Two launches, stream-ordered, no allocation, no synchronisation, capturable; a row
 * depends neither on B nor on its batch position.  The workspace holds lp [B][T][n_class] double, the chunk walks'
 * states [B][T][n_class] uint16 and chunk maps; its last 16 bytes receive two shader-cycle counts of row 0 (the
 * recurrence kernel, its backtrace parts) that tools/bench_pitch_tail.py reads and nothing else does. */
#define PD_RMVPE_VITERBI_CHUNK 32
int pd_rmvpe_viterbi_chunk(void);
size_t pd_rmvpe_viterbi_workspace_size(int B, int T, int n_class, int width);
int pd_rmvpe_viterbi(const float* hidden,      /* [B][T][n_class], device                            */
                     const double* log_band,   /* [n_class][2*width-1]: lt[i][j], column j-i+width-1 */
                     double log_off,           /* lt outside the band                                */
                     double log_init,          /* log of the initial state probability               */
                     long long* path,          /* [B][T], device                                     */
                     double* logp,             /* [B] or NULL                                        */
                     int B, int T, int n_class, int width, void* workspace, size_t ws_bytes, void* stream);
/* pd_rmvpe_viterbi for a ragged batch.  frames: device int32 [B]; row b's path runs over its first frames[b]
 * frames of hidden [B][T][n_class] (the row stride stays T): path[b][t] for t < frames[b] and logp[b] (of the
 * row's own last frame) equal pd_rmvpe_viterbi of those frames alone, path[b][t] = 0 for t >= frames[b].  The
 * frames past a row's length are never used by the recurrence (they may hold anything, NaN included).  A
 * frames[b] outside [1, T] is clamped into it.  frames == NULL returns PD_ERR_ARG; the workspace is that of
 * (B, T). */
int pd_rmvpe_viterbi_ragged(const float* hidden, const double* log_band, double log_off, double log_init,
                            long long* path, double* logp, const int* frames, int B, int T, int n_class, int width,
                            void* workspace, size_t ws_bytes, void* stream);

/* The f0 curve on another frame grid (component/pe/rmvpe.py:57-72: interp_f0, then resample_align_curve of the
 * curve and of its unvoiced flags, utils/pitch_utils.py:45-51, 86-98) for each row of f0 [B][n]:
 *   uv = f0 == 0; unvoiced frames take the linear interpolation of float32 log2 f0 between the neighbouring voiced
 *   frames (the first / last voiced value outside them, 0 for a row without a voiced frame), the curve is
 *   2^(float32 of that);  both the curve and uv (0.0 / 1.0) are interpolated from the grid j t_src onto i t_dst,
 *   i < m (m = the length of numpy.arange(0, (n - 1) t_src, t_dst), computed by the caller), then cut or padded with
 *   the last value to `length`;  uv_out = float32(uv curve) > 0.5;  f0_out = 0 where uv_out unless interp_uv.
 * Every interpolation is slope (x - xp[j]) + fp[j] in double without contraction, on numpy.interp's bracket, and is
 * rounded to float32 once.  n >= 2, m >= 1, length >= 1 (PD_ERR_ARG otherwise); n <= 262144 (PD_ERR_UNSUPPORTED).
 * f0_out [B][length] float32, uv_out [B][length] bytes (0 / 1).  One launch, one block per row, stream-ordered. */
int pd_f0_align(const float* f0, float* f0_out, unsigned char* uv_out, int B, int n, int m, int length, double t_src,
                double t_dst, int interp_uv, void* stream);
/* pd_f0_align for a ragged batch.  rows: device int32 [B][3] = (n_b, m_b, length_b) per row; f0 [B][n_stride],
 * f0_out [B][out_stride], uv_out [B][out_stride].  Row b is pd_f0_align of its first n_b source frames onto
 * length_b frames; f0_out[b][i] = 0 and uv_out[b][i] = 1 for i >= length_b.  The caller checks n_b >= 2,
 * m_b >= 1 and 1 <= length_b <= out_stride where it holds the values on the host; the kernel clamps n_b into
 * [2, n_stride], m_b to >= 1 and length_b into [0, out_stride] so that every access stays inside the row.
 * n_stride >= 2, out_stride >= 1, rows != NULL (PD_ERR_ARG otherwise); n_stride <= 262144. */
int pd_f0_align_ragged(const float* f0, float* f0_out, unsigned char* uv_out, const int* rows, int B, int n_stride,
                       int out_stride, double t_src, double t_dst, int interp_uv, void* stream);

/* ================================================================ harmonic-noise separation
 * pd_vr -- CascadedNet of modules/vr (nets.py, layers.py) with is_complex = True, its zero-padded STFT and its
 * iSTFT: what extract_harmonic_aperiodic runs on a vocoder output (handler/infer/handler.py:349-358) and on every
 * training utterance (component/binarizer/svs.py:113).  Inference only; fp32, with the convs on the bf16 MFMA as
 * an option of the handle (PD_VR_OPT_CONV_DTYPE below).
 *   frames:  n_frames = L / hop + 1, T = 32 (n_frames / 32 + 1), T_pad = (T - 1) hop - L, Tl_pad = (T_pad / 2 / hop) hop
 *            zeros on the left and the rest on the right; torch.stft(n_fft, hop, periodic Hann(n_fft), center = True,
 *            pad_mode = 'constant') of that has exactly T frames.  Frame t covers samples [t hop - lead, t hop - lead +
 *            n_fft) of the row with lead = n_fft / 2 + Tl_pad, zero outside [0, L).
 *   network: the input is cat([real, imag]) of the bins [0, n_fft / 2) (2 channels mono, re_L re_R im_L im_R stereo).
 *            BaseNet(nin, n): enc1 = conv3x3 + BN + ReLU; enc2..5 = two conv3x3 + BN + LeakyReLU(0.01), the first
 *            with stride 2, widths n (2, 4, 6, 8); ASPP (mean over the bins -> 1x1 conv repeated over the bins, a 1x1
 *            conv, three 3x3 convs dilated (4,2), (8,4), (12,6) as (bins, frames), concat, 1x1 bottleneck); dec4..2 =
 *            bilinear x2 (align_corners) cat skip -> conv3x3 + BN + ReLU; lstm_dec2 = 1x1 conv to one channel + BN +
 *            ReLU, a bidirectional LSTM over the frames (input = the bins, gate order i f g o, h_0 = c_0 = 0),
 *            Linear + BatchNorm1d + ReLU, appended as one channel; dec1.  The cascade: stage 1 on the low and the high
 *            half of the bins (BaseNet(nin, nout/2) + 1x1 conv to nout/4; BaseNet(nin, nout/4)), stage 2 on
 *            cat([band input, stage-1 output]) (widths nout and nout/2), stage 3 on cat([x, aux1, aux2]) over all
 *            bins, `out` (1x1, no bias), mask = tanh(|m|) m / (|m| + 1e-8) on the complex pairs, the last bin
 *            repeated once to n_fft / 2 + 1 bins.  T must be a multiple of 32, so that crop_center is the identity.
 *   inverse: torch.istft(spec * mask, n_fft, hop, Hann) and the samples [Tl_pad, Tl_pad + L) of it; the imaginary
 *            parts of the DC and Nyquist bins do not enter.
 * Every BatchNorm is the eval form (eps 1e-5), folded into its conv or Linear at create in double precision and
 * rounded once.  Spectra and masks cross the C-ABI as two planar f32 arrays [rows][T][n_fft / 2 + 1] (rows =
 * B * channels, row b * channels + c). */
typedef struct pd_vr pd_vr;

typedef struct {
  int n_fft;        /* 2048; a multiple of 64 in [64, 16384]                                               */
  int hop_length;   /* 512; >= 16, a divisor of n_fft other than n_fft itself (the squared-window overlap  */
                    /* sum reaches zero at hop = n_fft; torch.istft raises there too)                      */
  int nout;         /* 32; a multiple of 4 in [4, 256]                                                     */
  int nout_lstm;    /* 128; a multiple of 4 (the high-band nets halve it, the two directions halve it      */
                    /* again), at most 128: the recurrence kernel keeps a W_hh row of <= 64 hidden units   */
                    /* per direction in registers                                                          */
  int is_mono;      /* 0 (stereo model, 2 channels) or 1                                                   */
} pd_vr_dims;

/* Parameter order = the reference state-dict order without any num_batches_tracked: with cba(p) =
 * p.conv.0.weight, p.conv.1.{weight,bias,running_mean,running_var} and base(p) = cba(p.enc1), cba(p.encK.conv1),
 * cba(p.encK.conv2) for K = 2..5, cba(p.aspp.conv1.1), cba(p.aspp.conv2..5), cba(p.aspp.bottleneck),
 * cba(p.dec4.conv1), cba(p.dec3.conv1), cba(p.dec2.conv1), cba(p.lstm_dec2.conv),
 * p.lstm_dec2.lstm.{weight_ih_l0,weight_hh_l0,bias_ih_l0,bias_hh_l0} and the same four with the suffix _reverse,
 * p.lstm_dec2.dense.0.{weight,bias}, p.lstm_dec2.dense.1.{weight,bias,running_mean,running_var}, cba(p.dec1.conv1)
 * (114 tensors):
 *   base(stg1_low_band_net.0), cba(stg1_low_band_net.1), base(stg1_high_band_net), base(stg2_low_band_net.0),
 *   cba(stg2_low_band_net.1), base(stg2_high_band_net), base(stg3_full_band_net), out.weight, aux_out.weight
 * (582 tensors; aux_out is a training-time head and is not read), then the analysis and synthesis window [n_fft]
 * (the model's non-persistent `window` buffer, torch.hann_window(n_fft) in float32: the DFT tables are built from
 * these values, so that the frames at the edge of the zero padding, which see only the window's small ends, hold
 * what the reference's hold).  583 entries; 0 for dimensions outside the supported set. */
int pd_vr_num_params(const pd_vr_dims* dims);
/* Folds and packs every parameter and builds the DFT tables in the handle's weight pool on `stream`.  A dtype
 * other than PD_DTYPE_F32, or dimensions outside the ranges above, return PD_ERR_UNSUPPORTED before anything is
 * allocated. */
int pd_vr_create(const pd_vr_dims* dims, const float* const* params, int dtype, void* stream, pd_vr** out);
/* The caller must ensure that no call on the handle is still in flight. */
void pd_vr_destroy(pd_vr* h);
/* PD_VR_OPT_CONV_DTYPE = PD_DTYPE_F32 (the default) or PD_DTYPE_BF16: with bf16 every conv but the last (`out`)
 * rounds its input values to bf16 (nearest even; after the bilinear gather and the border's zeros, which stay f32)
 * and multiplies them with a bf16 copy of its folded weights on v_mfma_f32_32x32x16_bf16, accumulating in f32.
 * Bias, activation and every stored map stay f32, as do the STFT, the iSTFT, the LSTM and its two Linear layers,
 * the frequency mean, `out` and the bounded mask; workspace sizes do not change and an output row still depends
 * neither on the batch size nor on its position.  The first switch to bf16 builds the copy on `stream` inside the
 * handle's weight pool (pd_live_device_bytes counts it, pd_vr_destroy returns it); later switches only flip the
 * mode.  The caller must not switch while a call on the handle is in flight.  A null handle, an unknown option or
 * any other value returns PD_ERR_ARG. */
#define PD_VR_OPT_CONV_DTYPE 0
int pd_vr_set_option(pd_vr* h, int option, int value, void* stream);
/* T and lead (above) for a row of n_samples. */
int pd_vr_frames(const pd_vr* h, int n_samples);
int pd_vr_lead(const pd_vr* h, int n_samples);
/* Bytes pd_vr_separate needs for [B][channels][L]; pd_vr_mask on T frames needs those of L = (T - 32) hop. */
size_t pd_vr_workspace_size(const pd_vr* h, int B, int L);
/* The three stages.  All calls are stream-ordered, allocation-free and capturable; an output row depends neither
 * on the batch size nor on its position in the batch.
 * pd_vr_stft: wav [rows][L] -> re, im [rows][T][n_fft/2 + 1]. */
int pd_vr_stft(const pd_vr* h, const float* wav, float* re, float* im, int rows, int L, int lead, int T, void* stream);
/* pd_vr_mask: CascadedNet.forward.  spectrum -> mask, both [B channels][T][n_fft/2 + 1]; T a multiple of 32. */
int pd_vr_mask(const pd_vr* h, const float* spec_re, const float* spec_im, float* mask_re, float* mask_im, int B, int T,
               void* workspace, size_t ws_bytes, void* stream);
/* pd_vr_istft: y [rows][L_out] = the samples [lead - n_fft/2, lead - n_fft/2 + L_out) of torch.istft(spec * mask)
 * (mask_re = mask_im = NULL: of spec), which must lie inside its (T - 1) hop samples.  With resid non-NULL the same
 * epilogue writes resid = wav - y (wav [rows][L_out]). */
int pd_vr_istft(const pd_vr* h, const float* spec_re, const float* spec_im, const float* mask_re, const float* mask_im,
                const float* wav, float* y, float* resid, int rows, int T, int lead, int L_out, void* stream);
/* predict_from_audio: wav [B][channels][L] -> harmonic [B][channels][L], and aperiodic = wav - harmonic when
 * non-NULL.  The spectrum and the mask live in the workspace; nothing spectrum-sized is copied between the stages. */
int pd_vr_separate(const pd_vr* h, const float* wav, float* harmonic, float* aperiodic, int B, int L, void* workspace,
                   size_t ws_bytes, void* stream);
/* pd_vr_separate for a ragged batch.  lens: device int32 [B], row b's samples L_b in [1, L]; L (the longest row)
 * stays the row stride of wav, harmonic and aperiodic and sizes the workspace exactly as above.  Row b is computed
 * from its first L_b samples as the clip run alone: T_b = pd_vr_frames(L_b) frames with the lead pd_vr_lead(L_b) in
 * the STFT and the iSTFT; at U-Net level l every pixel with t >= T_b >> l lies outside the image, for every conv
 * (the ASPP's dilated taps and the frequency mean's 1x1 conv included: rows of 2, 4 and 6 bottom frames sit side by
 * side), the bilinear x2 gather's index and weight arithmetic uses the row's own heights, and both LSTM directions
 * run T_b / 2 trips, the reverse one from frame T_b / 2 - 1 and zero state.  Whatever wav holds past L_b, or the
 * workspace past T_b, is never used (it may be NaN).  harmonic[b][c][i] and aperiodic[b][c][i] for i < L_b equal,
 * bit for bit, pd_vr_separate of that row alone with L = L_b; for L_b <= i < L both are written as 0.  A lens[b]
 * outside [1, L] is clamped into it (every access stays inside the row).  lens == NULL returns PD_ERR_ARG.  The
 * launches are those of pd_vr_separate (a tile that lies wholly past its row's height returns at once, before any
 * barrier; the iSTFT's grid covers the L / hop + 2 segments a row of any length can have); stream-ordered, no
 * allocation, no synchronisation, capturable. */
int pd_vr_separate_ragged(const pd_vr* h, const float* wav, const int* lens, float* harmonic, float* aperiodic, int B,
                          int L, void* workspace, size_t ws_bytes, void* stream);
/* Its three stages.  pd_vr_stft_ragged and pd_vr_istft_ragged take lens: device int32 [rows], one sample count per
 * row (clamped into [1, L]); the row's frames and lead follow from it as pd_vr_frames and pd_vr_lead give them, so
 * the equal-length calls' `lead` has no counterpart.  T, a multiple of 32 that holds the frames of L samples, is the
 * row stride of the spectra; frames at or past a row's own count are neither written by the STFT nor read by the
 * iSTFT, which writes y (and resid) as 0 from the row's length up to L.
 * pd_vr_mask_ragged takes frames: device int32 [B], each a positive multiple of 32 and at most T (rounded down to a
 * multiple of 32 inside [32, T] otherwise); the mask past a row's frames is unspecified. */
int pd_vr_stft_ragged(const pd_vr* h, const float* wav, const int* lens, float* re, float* im, int rows, int L, int T,
                      void* stream);
int pd_vr_mask_ragged(const pd_vr* h, const float* spec_re, const float* spec_im, const int* frames, float* mask_re,
                      float* mask_im, int B, int T, void* workspace, size_t ws_bytes, void* stream);
int pd_vr_istft_ragged(const pd_vr* h, const float* spec_re, const float* spec_im, const float* mask_re,
                       const float* mask_im, const float* wav, const int* lens, float* y, float* resid, int rows, int T,
                       int L, void* stream);

/* ======================================================================== variance curves
 * pd_curves -- get_kth_harmonic, get_energy, get_voicing, get_breath and get_tension of
 * component/binarizer/binarizer_utils.py:115-213 (binarization: component/binarizer/svs.py:140-177; inference:
 * handler/infer/handler.py:352-358), with librosa 0.8.0's feature.rms and amplitude_to_db restated.  fp32 only.
 *   frames:   T = L / hop + 1 for a row of L samples, for the STFT (center = True) and the RMS alike.
 *   harmonic: f = f0 (k + 1), padded on the right with its last value to max(T_f0, T) frames; interp_f0 over all of
 *             it (log2 of the voiced frames, np.interp in double across the frames with f == 0, flat beyond the first
 *             and last voiced frame, rounded to f32, then exp2 of every frame; an all-unvoiced row keeps -inf, so
 *             f = 0); center = (f * win_size) / samplerate, start = max(center - hw, 0), end = min(center + hw,
 *             win_size / 2 + 1), bin i kept iff center >= 1 and start <= i < end, all in f32: at most 8 bins.  Only
 *             those bins of the STFT (reflect padding of win_size / 2, periodic Nuttall window) are computed, and the
 *             inverse is torch.istft's: the kept bins' sinusoids times the window, overlap-added and divided by the
 *             squared-window envelope of the frames that exist; DC and Nyquist enter with their real parts only.
 *             A frame without bins, and so an all-unvoiced row, gives exact zeros.
 *   rms:      the row padded by win_size / 2 on both sides (reflect, librosa 0.8.0, or zeros, librosa >= 0.10),
 *             frame t = padded [t hop, t hop + win_size), sqrt(mean(x^2)).
 *   finish:   the curve cut or zero-padded to mel_len; dB = max(d, max over the row of d - 80) with
 *             d = 10 log10(max(1e-10, S^2)); tension t = sqrt(max(E_full^2 - E_base^2, 0)) / (E_full + 1e-5),
 *             ratio: clip to [0, 1]; db: clip to [1e-5, 1], then dB; logit: clip to [1e-4, 1 - 1e-4], log(t / (1 - t));
 *             then the smoothing taps (cross-correlation, (k - 1) / 2 replicated frames on the left, the rest on the
 *             right: Conv1d padding = 'same', padding_mode = 'replicate'), then with `norm` clamp to [db_min, db_max]
 *             and (x - db_min) / (db_max - db_min).
 * Sums run in double and round once; the mask decision is f32 as above.  Rows of a batch have equal length in the
 * calls below; the *_ragged calls at the end of the section take per-row sizes. */
typedef struct pd_curves pd_curves;

typedef struct {
  int samplerate;     /* 44100; positive                                                                   */
  int win_size;       /* 2048; a multiple of 64 in [64, 4096]                                              */
  int hop_size;       /* 512; divides win_size, win_size / hop_size in [2, 16]                             */
  float half_width;   /* 3.5; in (0, 3.5], so that at most 8 bins survive                                  */
} pd_curves_dims;

#define PD_CURVES_PAD_REFLECT 0
#define PD_CURVES_PAD_CONSTANT 1
#define PD_CURVES_AMPLITUDE 0
#define PD_CURVES_DB 1
#define PD_CURVES_TENSION_RATIO 0
#define PD_CURVES_TENSION_DB 1
#define PD_CURVES_TENSION_LOGIT 2

/* Builds the window and the win_size-entry cos / sin table in double precision, rounded once to f32.  Dimensions
 * outside the ranges above return PD_ERR_ARG, the message naming the value, before anything is allocated. */
int pd_curves_create(const pd_curves_dims* dims, void* stream, pd_curves** out);
/* The caller must ensure that no call on the handle is still in flight. */
void pd_curves_destroy(pd_curves* h);
/* T for a row of n_samples; 0 for a null handle or n_samples <= win_size / 2 (reflect padding needs more). */
int pd_curves_frames(const pd_curves* h, int n_samples);
/* Bytes any call below needs for B rows of L samples and T_f0 f0 frames (0 where the call takes no f0). */
size_t pd_curves_workspace_size(const pd_curves* h, int B, int L, int T_f0);
/* All calls are stream-ordered, allocation-free and capturable; an output row depends neither on the batch size nor
 * on its position in the batch.  `taps` is a device array of kernel_size in [3, 257] floats, or NULL: no smoothing.
 * pd_curves_kth_harmonic: wav [B][L], f0 [B][T_f0] in Hz (0 = unvoiced), k >= 0 -> y [B][L], and with resid
 * non-NULL resid = wav - y from the same epilogue. */
int pd_curves_kth_harmonic(const pd_curves* h, const float* wav, const float* f0, int k, float* y, float* resid, int B,
                           int L, int T_f0, void* workspace, size_t ws_bytes, void* stream);
/* get_energy / get_voicing / get_breath: wav [B][L] -> out [B][mel_len]; domain PD_CURVES_AMPLITUDE or PD_CURVES_DB. */
int pd_curves_energy(const pd_curves* h, const float* wav, int pad_mode, int domain, int mel_len, const float* taps,
                     int kernel_size, int norm, float db_min, float db_max, float* out, int B, int L, void* workspace,
                     size_t ws_bytes, void* stream);
/* SinusoidalSmoothingConv1d.forward on any taps: x [rows][T] -> out [rows][T]. */
int pd_curves_smooth(const float* x, const float* taps, int kernel_size, float* out, int rows, int T, void* stream);
/* The fused call: sp, ap [B][L], f0 [B][T_f0] -> voicing, breath, tension [B][mel_len]; rms(sp) is computed once for
 * voicing and tension.  voicing and breath (with ap) may be NULL: get_tension alone.  base non-NULL: the base
 * harmonic [B][L] (k = 0) is returned too.  norm, db_min, db_max apply to voicing and breath. */
int pd_curves_forward(const pd_curves* h, const float* sp, const float* ap, const float* f0, int pad_mode,
                      int tension_domain, int mel_len, const float* taps, int kernel_size, int norm, float db_min,
                      float db_max, float* voicing, float* breath, float* tension, float* base, int B, int L, int T_f0,
                      void* workspace, size_t ws_bytes, void* stream);
/* The three calls above for a ragged batch.  rows: device int32 [B][3] = (L_b, mel_len_b, T_f0_b) per row (a call
 * that takes no f0, or no mel_len, ignores that value); L, mel_len and T_f0 stay the row strides of the waveforms,
 * the curves and f0 and size the workspace.  Row b is that row run alone: the reflect or constant padding at its own
 * end, T_b = L_b / hop + 1 frames, f0 padded on the right with its last value and interpolated over its own T_f0_b
 * frames, amplitude_to_db's maximum over its own mel_len_b frames, the smoothing's edge clamp at mel_len_b.  What
 * the inputs hold past a row's sizes is never used (it may be NaN).  The outputs below mel_len_b and L_b equal, bit
 * for bit, the equal-length call of that row alone; past them they are written as 0.  Each L_b must exceed
 * win_size / 2 and lie in (win_size / 2, L], mel_len_b in [1, mel_len], T_f0_b in [1, T_f0]: the caller checks this
 * where it holds the values on the host, the kernels clamp into these ranges so that every access stays inside the
 * row.  rows == NULL returns PD_ERR_ARG.  Same launches as the equal-length calls (a block that lies wholly past its
 * row's frames returns at once, before any barrier); stream-ordered, no allocation, capturable. */
int pd_curves_kth_harmonic_ragged(const pd_curves* h, const float* wav, const float* f0, int k, float* y, float* resid,
                                  const int* rows, int B, int L, int T_f0, void* workspace, size_t ws_bytes,
                                  void* stream);
int pd_curves_energy_ragged(const pd_curves* h, const float* wav, int pad_mode, int domain, int mel_len,
                            const float* taps, int kernel_size, int norm, float db_min, float db_max, float* out,
                            const int* rows, int B, int L, void* workspace, size_t ws_bytes, void* stream);
int pd_curves_forward_ragged(const pd_curves* h, const float* sp, const float* ap, const float* f0, int pad_mode,
                             int tension_domain, int mel_len, const float* taps, int kernel_size, int norm,
                             float db_min, float db_max, float* voicing, float* breath, float* tension, float* base,
                             const int* rows, int B, int L, int T_f0, void* workspace, size_t ws_bytes, void* stream);

/* ================================================================ FastDiff analysis
 * process_utterance (utils/data_gen_utils.py:95-149), the analysis half of the FastDiff vocoder
 * (component/vocoder/fastdiff.py:128-145): an optional loudness normalisation (pyloudnorm's ITU-R BS.1770 meter),
 * librosa.stft centred with pad_mode="constant", a linear-magnitude Slaney mel (logged only for vocoder='pwg') and
 * the waveform padded to T hop samples.
 *
 * pd_mel_create_centered_zero -- a third constructor of pd_mel: zero padding of nf/2 samples on both sides,
 * T = 1 + L / hn frames, frame t centred on sample t hn, min_samples 1.  out_mode selects what pd_mel_forward
 * writes: out_scale * log(max(mel, clip_val)) as the other constructors (PD_MEL_OUT_LN), out_scale * mel
 * (PD_MEL_OUT_LINEAR, vocoder='fastdiff') or out_scale * log10(max(mel, clip_val)) (PD_MEL_OUT_LOG10, 'pwg' with
 * clip_val = eps).  Window, key shift, bins, basis, spec_out and lens are as pd_mel_create; what a row holds past
 * lens[b] is never read. */
#define PD_MEL_OUT_LN 0
#define PD_MEL_OUT_LINEAR 1
#define PD_MEL_OUT_LOG10 2
int pd_mel_create_centered_zero(const pd_mel_dims* dims, const float* mel_basis, int out_mode, void* stream,
                                pd_mel** out);
/* return_linear's spectrum (utils/audio.py:51-56): out[i] = (20 log10(max(1e-5, spec[i])) - min_level_db) /
 * (-min_level_db), i < n, in f32; min_level_db < 0.  out may alias spec. */
int pd_mel_normalize_spec(const float* spec, float min_level_db, float* out, size_t n, void* stream);

/* pd_loudness -- Meter(rate).integrated_loudness and normalize.loudness of pyloudnorm, mono, with the peak step of
 * process_utterance :121-122.  The K-weighting is two biquads (a high shelf, then a high pass) whose coefficients
 * the caller designs in double (prodiff_amd.analysis.kweighting_coefficients) and passes normalised (a[0] = 1);
 * they run as scipy.signal.lfilter's direct form II transposed, in fp64, each row cut into chunks of
 * pd_loudness_chunk() samples: a chunk's zero-state response, a scan of the chunks' end states with the four
 * states' transition over one chunk, then each chunk again from its true initial state.  Block j covers the
 * samples [bounds[j][0], min(bounds[j][1], L_b)); its energy is the sum of y^2 in double times 1 / (0.4 rate).
 * The gates: l_j = -0.691 + 10 log10 z_j; absolute l_j >= -70; relative l_j > G_r and l_j > -70 with
 * G_r = -0.691 + 10 log10(mean z over the absolute gate) - 10; the loudness is -0.691 + 10 log10(mean z over both
 * gates), -inf when no block passes.  Every sum's order is fixed by the chunk size, the bounds and the row's own
 * length: row b of a batch equals that row run alone, bit for bit.  Samples must be finite. */
typedef struct pd_loudness pd_loudness;

typedef struct {
  int rate;             /* Hz, in [1000, 768000]                                      */
  double shelf_b[3];    /* high shelf: +4 dB, Q = 1/sqrt(2), 1500 Hz                  */
  double shelf_a[3];    /* a[0] = 1                                                   */
  double pass_b[3];     /* high pass: Q = 0.5, 38 Hz                                  */
  double pass_a[3];     /* a[0] = 1                                                   */
} pd_loudness_dims;

/* Nothing is allocated on the device.  Unstable or unnormalised coefficients return PD_ERR_ARG. */
int pd_loudness_create(const pd_loudness_dims* dims, void* stream, pd_loudness** out);
void pd_loudness_destroy(pd_loudness* h);
/* Samples per chunk of the recurrence. */
int pd_loudness_chunk(void);
/* ceil(0.4 rate): pyloudnorm refuses a shorter signal. */
int pd_loudness_min_samples(const pd_loudness* h);
size_t pd_loudness_workspace_size(const pd_loudness* h, int B, int L, int n_blocks);
/* wav [B][L], lens int32 [B] or NULL -> loud_out double [B]; peak_out float [B] = max |x| of each row, or NULL;
 * wav_out [B][L_out] or NULL = f32(10^((target - loudness) / 20)) * x in f32, divided by its own maximum when
 * that exceeds 1, and 0 from the row's length up to L_out (librosa_pad_lr and the trim to T hop when L_out is
 * (1 + L / hop) hop).  bounds: device int32 [n_blocks][2], the block bounds the host evaluated; counts: device
 * int32 [B], the blocks of each row (<= n_blocks).  The caller checks on the host that every row holds at least
 * pd_loudness_min_samples; the kernels clamp lens, counts and bounds so that every access stays inside the row.
 * L < pd_loudness_min_samples returns PD_ERR_ARG.  Six launches, stream-ordered, no allocation. */
int pd_loudness_forward(const pd_loudness* h, const float* wav, const int* lens, const int* bounds, const int* counts,
                        int n_blocks, double target, double* loud_out, float* peak_out, float* wav_out, int B, int L,
                        int L_out, void* workspace, size_t ws_bytes, void* stream);
/* out [B][L_out] = the row's first min(lens[b], L) samples, then zeros: the padding alone (loud_norm off). */
int pd_loudness_pad(const float* wav, const int* lens, float* out, int B, int L, int L_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PRODIFF_HIP_H */
