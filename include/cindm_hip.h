/*
 * cindm_hip.h -- C ABI of libcindm_hip.so: MI355X (gfx950) implementation of CinDM's
 * compositional diffusion SAMPLING hot path.
 *
 * The upstream reference (AI4Science-WestlakeU/cindm) has no native/FFI layer: its callers
 * construct Python classes and call methods.  Each entry point below therefore cites the
 * reference *Python* interface (file:line relative to the reference root) whose arithmetic
 * it replaces; the Python face in cindm_amd/ keeps those class/method signatures and binds
 * to this library through ctypes (see INTEGRATION.md for the binding stub).
 *
 * Conventions
 *   - every function returns int: 0 = OK, <0 = error; text via cindm_last_error() (thread-local)
 *   - no C++ types / exceptions cross the boundary; no torch types in any signature
 *   - the CALLER owns every tensor buffer and the workspace and passes raw DEVICE pointers plus
 *     explicit sizes; the library owns only opaque handles and its packed copies of the weights
 *   - all launches are asynchronous on the hipStream_t passed in (as void*); nothing
 *     synchronises the device except *_finalize
 *   - a handle is bound to the device current at *_create and is not thread-safe
 *   - all tensors are fp32, contiguous, layout [batch, time, feature] (the reference's API
 *     layout, model/diffusion_1d.py:610-614), which is also the channel-last layout the kernels
 *     use internally
 */
#ifndef CINDM_HIP_H
#define CINDM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point's argument list changes or an entry point is added.  History: 1 = rounds 1-2; 2 = round 3's
 * positional sum_boundary argument of cindm_airfoil_design_grad / cindm_ddpm2d_sample_force, and round 4's additions
 * (cindm_unet1d_poll, cindm_ddpm2d_predict, cindm_unet1d_phase_prof_*, option "no_exchange", cindm_unet1d_recovered).
 * A caller compiled against another version must not bind: compare cindm_abi_version() with this constant. */
#define CINDM_ABI_VERSION 4

typedef struct cindm_unet1d cindm_unet1d;
typedef struct cindm_ddpm1d cindm_ddpm1d;

/* ------------------------------------------------------------------ misc */
int cindm_abi_version(void);
const char* cindm_last_error(void);
/* sha256 (hex) of the sources this library was compiled from (everything under cindm_amd/csrc plus this header), embedded by
 * cindm_amd/build.py: the Python face refuses a library whose hash differs from the sources next to it. */
const char* cindm_source_hash(void);

/* In-kernel phase clocks of the persistent 2-D convolution kernel (cindm_amd/csrc/kernels2d_v2.h), profiling build only
 * (libcindm_hip_prof.so): copies [8 categories][2 roles][8 phases] sums of 10 ns ticks (128 words) to dst and clears them.
 * Returns 1 in the profiling build, 0 in the production build (zeros), -1 on error.  No reference counterpart (a tool). */
int cindm_ws_prof_read(unsigned long long* dst);

/* ------------------------------------------------------------------ TemporalUnet1D
 * Replaces TemporalUnet1D.__init__/forward, model/diffusion_1d.py:517-646, and the blocks it
 * is built from: SinusoidalPosEmb :146, Conv1dBlock :197, ResidualTemporalBlock :483,
 * Residual/PreNorm/LayerNorm/LinearAttentionTemporal :75/:134/:123/:272, Downsample1d :92,
 * Upsample1d :100. */
typedef struct {
    int32_t horizon;          /* TemporalUnet1D(horizon=...)           :521 */
    int32_t transition_dim;   /* n_bodies * 4 features                 :522 */
    int32_t dim;              /* base width: a power of two >= 32 (64: the n-body checkpoints), or 96 (the
                                 "Unet_dim-96" checkpoint; GroupNorm groups of 12 / 24 / 48 / 96 channels, served by the
                                 generic kernels only: three launches per block and per attention site).  Any other width
                                 is refused at create with "dim must be a power of two >= 32 or 96"      :524 */
    int32_t n_mults;          /* len(dim_mults), <= 8                  :525 */
    int32_t dim_mults[8];     /* powers of two */
    int32_t attention;        /* 0/1                                   :526 */
    int32_t timesteps;        /* size of the per-timestep bias table (diffusion T, 1000) */
} cindm_unet1d_desc;

int  cindm_unet1d_create(const cindm_unet1d_desc* desc, cindm_unet1d** out);
void cindm_unet1d_destroy(cindm_unet1d* h);

/* State-dict manifest (the reference's nn.Module.state_dict() key names, registration order,
 * SURVEY.md Appendix A.3): number of tensors; name/shape of tensor idx. */
int  cindm_unet1d_num_params(const cindm_unet1d* h);
int  cindm_unet1d_param_info(const cindm_unet1d* h, int idx, char* name, int name_cap,
                             int64_t shape[4], int* ndim);
/* Copy one state-dict tensor (PyTorch layout, fp32) into the handle; src may be a host
 * (on_device=0) or device (on_device=1) pointer.  Replaces load_state_dict for this module. */
int  cindm_unet1d_set_param(cindm_unet1d* h, const char* key, const float* src, int64_t numel,
                            int on_device);
/* Optional: sinusoidal embedding table [timesteps, dim] (host fp32), row t = SinusoidalPosEmb(t)
 * (:151-158).  If never called, *_finalize computes it with libm expf/sinf/cosf. */
int  cindm_unet1d_set_sinusoid_table(cindm_unet1d* h, const float* table_host, int64_t numel);
/* Repack weights to the kernels' [tap][Cin][Cout] layout and precompute, for every timestep,
 * the time path time_mlp -> per-block Mish->Linear biases (:537-542, :493-497, :509) with the
 * GEMM kernels.  Synchronises `stream`.  On all three model handles *_finalize returns at once when the handle is finalized
 * already (no parameter, sinusoid table or pack option changed since its last finalize), and *_workspace_bytes returns 0 for a
 * handle that is not finalized. */
int  cindm_unet1d_finalize(cindm_unet1d* h, void* stream);

/* Kernel-path selection for this handle.  The options of the three model handles are of three kinds:
 *   pack options select what *_finalize packs: changing one un-finalizes the handle (the next *_finalize repacks);
 *   run-time options select among kernels whose operands are packed already: the handle stays finalized --
 *     cindm_unet1d: "no_exchange", "recover", "tune";  cindm_unet2d: none;  cindm_forceunet: "no_exchange", "recover", "dbg", "stress";
 *   "range_fallback" is read-only: *_set_option refuses it as an unknown key ("unknown option: range_fallback").
 * Every alternative path computes the same function (the parity suite runs all of them); defaults are the fast path.  Keys (25; DESIGN.md section 4.6 lists what round 6 removed and why):
 *   "mfma_f32" (1 = exact fp32 MFMA kernels instead of the split-fp16 ones), "local_gn", "attn_site", "attn_head" (0 / 1 / 2),
 *   "level0" (master switch of the level kernels), "level1" (0 / 1 / 2 samples per workgroup), "ups_last", "ups_tail",
 *   "level_pairs" (1 = up to 320 rows the two finest down levels run as one launch and so do the two finest up levels, when both stand-alone
 *   level kernels of a pair would run: two launches fewer per forward, bit-identical results), "dconv", "dconv2",
 *   "dresample" (0 / 1 / 2: general kernel / 32 / 16-or-32 columns per workgroup), "l2_prefetch" (launches touch their successor's weights), "ws_alias", "pingpong" (the sample loops keep t / step index /
 *   epochs in two slots advanced by the step's update), "fuse_update" (plain single-model steps apply the update inside the last U-Net
 *   kernel), "fuse_gather" (time composition of two-body states: the first U-Net kernel reads the state's windows in place),
 *   "taps" (1 = block outputs that live only inside a level kernel are also stored for cindm_unet1d_tap; off on the sampling path),
 *   "auto_range" (1 = the range rule: a checkpoint outside the split-fp16 window runs on the fp32 kernels), "range_fallback" (read-only:
 *   1 a weight left the window 2^-12 <= max|w| <= 2^15, 2 the calibration batch overflowed, 3 the caller's own batch did --
 *   cindm_unet1d_range_escalate), "no_exchange", "recover", "stress", "tune" (same-box A/B word: bit 0 = round 5's L2 warm-up placement,
 *   regions and issuers, bit 1 = round 5's plain output stores, bit 2 + i = launch i of the forward issues no warm-up), "dbg" (timing ablations / forced time-outs: wrong results).
 * No reference counterpart (PyTorch picks its own kernels). */
int  cindm_unet1d_set_option(cindm_unet1d* h, const char* key, int32_t value);
int  cindm_unet1d_get_option(const cindm_unet1d* h, const char* key, int32_t* value);

/* Synchronises `stream` and reports a device-side fault of earlier forwards (the bounded in-kernel exchange between
 * workgroup pairs of the C = 512 GroupNorms timing out).  0 = healthy. */
int  cindm_unet1d_status(cindm_unet1d* h, void* stream);
/* The same check for callers that recover: 0 = healthy, 1 = an exchange of an earlier forward on `stream` timed out (its results
 * are invalid; the flag is cleared), < 0 = error.  Recovery = set_option("no_exchange", 1), re-issue the work, set it back: with
 * "no_exchange" the forward runs on the kernels that exchange nothing between workgroups (per-layer conv_gemm_h3 launches with
 * consumer-side GroupNorm at C = 512, the one-workgroup attention site kernel), which cannot time out.  "no_exchange" is a
 * RUN-TIME option: it does not un-finalize the handle.  The sample loops (cindm_ddpm1d_sample / _sample_ddim / _sample_guided)
 * do this by themselves: a chain whose exchange timed out (foreign load on the device kept a partner workgroup from becoming
 * resident) is re-run ONCE from its initial state on the exchange-free kernels; cindm_unet1d_recovered() counts those re-runs. */
int  cindm_unet1d_poll(cindm_unet1d* h, void* stream);
int  cindm_unet1d_recovered(const cindm_unet1d* h);
/* The range rule on the caller's own data (ABI 4): on = 1 repacks a handle that runs the split-fp16 kernels for the exact fp32-MFMA
 * kernels ("range_fallback" then reads 3) -- called by the Python face when the FIRST forward / chain after a weight synchronisation
 * returns inf / nan; on = 0 undoes exactly that.  Synchronises the stream and repacks the weights as cindm_unet1d_finalize does (a
 * finalisation step, not part of a chain's steady state: at most once per weight synchronisation). */
int  cindm_unet1d_range_escalate(cindm_unet1d* h, int32_t on, void* stream);
/* Profiling builds only (cindm_amd/build.py --prof: -DCINDM_PHASE_PROF -> libcindm_hip_prof.so): per-launch, per-workgroup,
 * per-wave phase clocks (s_memrealtime, 100 MHz) of the level kernels, dconv2_kernel, dresample_kernel and attn1d_head_kernel.
 * enable: (re)allocates the record buffer and arms it for every following forward of this handle (inside graph replays too);
 * read: copies the records of the LAST forward/replayed step, [launch slot][workgroup < 1024][wave < 8][16 stamps] uint64,
 * into host memory (dst_cap in uint64 words) and returns the number of launch slots used (names via cindm_unet1d_phase_prof_name).
 * In a production build enable returns -1 ("not a profiling build"). */
int  cindm_unet1d_phase_prof_enable(cindm_unet1d* h, int32_t on);
int  cindm_unet1d_phase_prof_read(cindm_unet1d* h, unsigned long long* dst, int64_t dst_cap, void* stream);
const char* cindm_unet1d_phase_prof_name(const cindm_unet1d* h, int32_t slot);

size_t cindm_unet1d_workspace_bytes(const cindm_unet1d* h, int64_t rows);
/* eps[rows,horizon,F] = TemporalUnet1D.forward(x[rows,horizon,F], time=t)   (:610-646).
 * All rows share timestep t (as every caller on the sampling path does).  If t_dev != NULL the
 * timestep is read from that device int32 at kernel run time (graph-replayable) and t is ignored. */
int  cindm_unet1d_forward(cindm_unet1d* h, const float* x, int32_t t, const int32_t* t_dev,
                          float* eps, int64_t rows, void* ws, size_t ws_bytes, void* stream);
/* Debug/parity aid: copy a named intermediate activation of the LAST forward (same rows/ws)
 * to dst (device, capacity dst_cap floats) in channel-last layout [rows, L, C].
 * Names: reference module paths, e.g. "downs.0.0", "mid_attn", "ups.2.3", "final_conv.0". */
int  cindm_unet1d_tap(cindm_unet1d* h, const char* name, int64_t rows, void* ws, float* dst,
                      int64_t dst_cap, int64_t shape[3], void* stream);
/* Instrumented forward for bench.py's roofline leg: as cindm_unet1d_forward, but every launch is
 * issued 8 times back-to-back (launches are idempotent) inside one pair of HIP events recorded on `stream`,
 * the bracket time divided by 8 being the launch's duration (this amortises the ~6 us cost of an event
 * bracket and includes the dependent-launch gap a kernel also pays inside the sampling graph); returns per kernel kind k
 * (0..4 = conv_gemm_kernel<T> for T = 0,1,3,4,5; 5 = linattn_core_kernel) the launch count, the summed
 * duration in ms and the summed ALGORITHMIC FLOPs (2*M*N*K of the layer, no padding).
 * Synchronises `stream`. */
int  cindm_unet1d_profile(cindm_unet1d* h, const float* x, int32_t t, float* eps, int64_t rows,
                          void* ws, size_t ws_bytes, void* stream,
                          int32_t counts[6], float ms[6], double flops[6]);
/* Same, one record per launch in issue order (at most cap): kernel kind, duration ms, algorithmic FLOPs,
 * and (grid.x, grid.y, pipeline stages) triples. */
int  cindm_unet1d_profile_detail(cindm_unet1d* h, const float* x, int32_t t, float* eps, int64_t rows,
                                 void* ws, size_t ws_bytes, void* stream, int32_t cap, int32_t* n_out,
                                 int32_t* kind, float* ms, double* flops, int32_t* grid_xy_stages);
/* Number of kernel launches one forward issues (for DESIGN/bench bookkeeping). */
int  cindm_unet1d_launches_per_forward(const cindm_unet1d* h);

/* ------------------------------------------------------------------ GaussianDiffusion1D (sampling half)
 * Replaces GaussianDiffusion1D.model_predictions :951, gradient :1857, p_mean_variance :1033,
 * q_posterior :938, predict_start_from_noise :914, p_sample :1047, p_sample_compose_inside :1190,
 * p_sample_compose_outside :1380, p_sample_loop :1656, sample_compose_multibodies :1986 (both phases),
 * sample_step_ULA :2048, q_sample :2399 of model/diffusion_1d.py. */
typedef struct {
    int32_t timesteps;
    /* the 13 fp32 buffers registered at :873-910, host pointers, each [timesteps] */
    const float* betas;
    const float* alphas_cumprod;
    const float* alphas_cumprod_prev;
    const float* sqrt_alphas_cumprod;
    const float* sqrt_one_minus_alphas_cumprod;
    const float* log_one_minus_alphas_cumprod;
    const float* sqrt_recip_alphas_cumprod;
    const float* sqrt_recipm1_alphas_cumprod;
    const float* posterior_variance;
    const float* posterior_log_variance_clipped;
    const float* posterior_mean_coef1;
    const float* posterior_mean_coef2;
    const float* loss_weight;
} cindm_sched_desc;

int  cindm_ddpm1d_create(const cindm_sched_desc* desc, cindm_ddpm1d** out);
void cindm_ddpm1d_destroy(cindm_ddpm1d* h);

enum {
    CINDM_COMPOSE_PLAIN = 0,          /* self.model(x) on the whole state                  :1006 */
    CINDM_COMPOSE_MEAN_INSIDE = 1,    /* compose_mode "mean-inside"                        :994-996 */
    CINDM_COMPOSE_SUM_INSIDE = 2,     /* compose_mode "sum-inside"                         :997-999 */
    CINDM_COMPOSE_MEAN_OUTSIDE = 3,   /* p_sample_compose_outside compose_mode "mean"      :1447-1452 */
    CINDM_COMPOSE_NOISESUM_OUTSIDE = 4, /* compose_mode "noise_sum"                        :1453-1463 */
    CINDM_COMPOSE_MULTIBODY = 5       /* gradient(): pair model + unconditioned model      :1865-1926 */
};
enum { CINDM_OBJ_PRED_NOISE = 0, CINDM_OBJ_PRED_X0 = 1, CINDM_OBJ_PRED_V = 2 };

typedef struct {
    int32_t mode;               /* CINDM_COMPOSE_* */
    int32_t n_windows;          /* n_composed + 1                                          :977 */
    int32_t compose_start_step; /* window stride                                           :978 */
    int32_t window;             /* single_model_step = image_size                          :963 */
    int32_t n_bodies;           /* compose_n_bodies (state feature dim = 4*n_bodies)       :964 */
    int32_t cond_steps;         /* conditioned_steps: rows of `cond` prepended to x        :956-957 */
    int32_t objective;          /* CINDM_OBJ_*                                             :1010-1027 */
    int32_t clip_denoised;      /* x_start.clamp_(-1,1)                                    :1038-1039 */
    float   uncond_coef;        /* coefficient_unconditioned_grad = 1.4 (MULTIBODY)        :1900 */
} cindm_compose_desc;

/* Bytes of the step workspace: the U-Net inputs / predictions of a composed step, the U-Net workspace(s), the guided step's
 * staging, AND (ABI 4) the chain-level buffers of the sample loops -- the x_T snapshot the exchange-time-out recovery re-runs
 * from (B * L_tot * F floats) and the DDIM loop's per-step tables (5 words per U-Net timestep).  Nothing is allocated after
 * *_create / *_finalize: no entry point below calls hipMalloc / hipFree (asserted by a CPU test over the sources). */
size_t cindm_ddpm1d_workspace_bytes(const cindm_ddpm1d* h, const cindm_unet1d* pair,
                                    const cindm_unet1d* uncond, const cindm_compose_desc* c, int64_t B);

/* p_mean_variance (:1033-1044) for one timestep: evaluate the composed U-Nets on x
 * [B, L_tot, 4*n_bodies] (with cond [B, cond_steps, F] prepended when cond_steps > 0), aggregate
 * eps over windows / body pairs, x0 = predict_start_from_noise, clamp, posterior mean.
 * Writes mean_out, x0_out, eps_out (each [B, L_tot, F], any may be NULL). */
int  cindm_ddpm1d_predict(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                          const cindm_compose_desc* c, const float* x, const float* cond,
                          int32_t t, const int32_t* t_dev, int64_t B,
                          float* mean_out, float* x0_out, float* eps_out,
                          void* ws, size_t ws_bytes, void* stream);

/* One full reverse step without design guidance (p_sample :1061-1120 / p_sample_compose_inside
 * :1209-1283 / p_sample_compose_outside :1406-1523 with design_fn=None):
 *   x <- mean + exp(0.5*logvar_t) * z   (z = 0 at t == 0), in place.
 * z = noise[B,L_tot,F] if noise != NULL, else the library's counter-based Gaussian
 * keyed by (seed, sample_offset + b, t, element).
 * Inpainting (:1715-1718): if inpaint_cond != NULL, afterwards
 *   x[:, :inpaint_steps] = q_sample(inpaint_cond, t, inpaint_noise or counter-based noise). */
int  cindm_ddpm1d_step(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                       const cindm_compose_desc* c, float* x, const float* cond,
                       const float* noise, uint64_t seed, int64_t sample_offset,
                       const float* inpaint_cond, int32_t inpaint_steps, const float* inpaint_noise,
                       int32_t t, const int32_t* t_dev, int64_t B, float* x0_out,
                       void* ws, size_t ws_bytes, void* stream);

/* The reverse loop (p_sample_loop :1682-1720 / sample_compose_multibodies :2000-2033 without
 * design guidance): for t = t_start, t_start-1, ..., t_end: cindm_ddpm1d_step.  One step is
 * captured into a hipGraph (timestep held in a device counter) and replayed.
 * noise_steps: NULL (counter-based noise) or device tensor [timesteps, B, L_tot, F] indexed by t;
 * inpaint_noise_steps likewise [timesteps, B, inpaint_steps, F]. */
int  cindm_ddpm1d_sample(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                         const cindm_compose_desc* c, float* x, const float* cond,
                         const float* noise_steps, uint64_t seed, int64_t sample_offset,
                         const float* inpaint_cond, int32_t inpaint_steps,
                         const float* inpaint_noise_steps,
                         int32_t t_start, int32_t t_end, int64_t B,
                         void* ws, size_t ws_bytes, void* stream, int32_t use_graph);

/* Built-in design objective: the paper's point objective (inference/inverse_design_diffusion_1d.py:211-229),
 *   "L2":       coef * sum_bodies sum_b mean_{last n steps} || pos - target ||_2
 *   "L2square": coef * sum_bodies sum_b mean_{last n steps} || pos - target ||_2^2
 *   (+ time_consistency_coef * sum_b mean_l || pos[l+1] - pos[l] ||^2 over the position channels),
 * whose gradient with respect to the state is evaluated in closed form inside the update kernel.
 * Modes 3 / 4 are the waypoint objective, the same two norms read from device tables (cindm_ddpm1d_set_design_tables below):
 *   sum_b sum_l sum_j scale[b | 0, l, j] * || pos[b, l, 4j : 4j+2] - target[b | 0, l, j] ||_2     (mode 4: ||.||_2^2)
 *   (+ the time-consistency term); in these modes last_n_step, coef and pos_target are not read.
 * Mode 5 is the quadratic objective, read from device tables as well (cindm_ddpm1d_set_design_quadratic below):
 *   sum_b sum_l ( 1/2 x[b, l]^T S[b | 0, l] x[b, l] - h[b | 0, l]^T x[b, l] )     over all F = 4 * n_bodies features of a row
 *   (+ the time-consistency term, on the position channels); last_n_step, coef and pos_target are not read either.
 * Mode 6 is the pair-distance objective, read from device tables as well (cindm_ddpm1d_set_design_pairdist below):
 *   sum_b sum_l sum_p weight[b | 0, l, p] * ( max(lo[b | 0, l, p] - r, 0)^2 + max(r - hi[b | 0, l, p], 0)^2 )
 *   with r the distance between the positions of the bodies of pair p at row l (+ the time-consistency term); last_n_step, coef and
 *   pos_target are not read either.
 * Mode 7 is the sum of every kind of table armed on the handle, at least one: the values of modes 3 | 4, 5 and 6 added, with the
 *   time-consistency term once.  The three setters arm the terms; each armed kind is checked against the state as under its own mode.
 *   The update evaluates each present term as that mode's own kernel does and adds them in the order quadratic, waypoint,
 *   pair-distance, each sum rounded once (compose_update_sum_kernel; a sum of one kind is that kind's mode bit for bit).  In mode 7
 *   last_n_step is not a row count: it names the waypoint term's norm, 1 = "L2", 2 = "L2square" (the point modes' numbering); it is
 *   ignored when no waypoint tables are armed and any other value is refused when they are.  coef and pos_target are not read. */
typedef struct {
    int32_t mode;               /* 1 = "L2", 2 = "L2square"; 3 = table "L2", 4 = table "L2square"; 5 = quadratic tables; 6 = pair-distance tables; 7 = the sum of the tables armed */
    int32_t alpha;              /* 0: "standard" (gradient as is), 1: "standard-alpha" (x eta_t)   :1243-1248 */
    int32_t recurrence;         /* 0: non-recurrence branch; N >= 1: "-recurrence-N"                :1284-1370 */
    int32_t last_n_step;
    float   coef;
    float   time_consistency_coef;
    float   pos_target[2];
} cindm_design_desc;

/* The reverse loop WITH design guidance by the built-in objective ("standard" / "standard-alpha", optionally
 * "-recurrence-N"; p_sample :1061-1186, p_sample_compose_inside :1209-1370, p_sample_compose_outside :1406-1652):
 * per step, max(N, 1) x [ p_mean_variance; pred = mean - [eta_t] grad objective(x); overwrite the first
 * overwrite_steps rows with initial_state_overwrite [B, overwrite_steps, F] if given; relaxation
 * x <- sqrt(abar_t/abar_{t-1}) pred + sqrt(1 - abar_t/abar_{t-1}) z' ] with the last iteration's
 * pred + sigma_t z as the result -- all inside the captured step, no host code in the loop.
 * recur_noise_steps: NULL (counter-based) or [timesteps, max(N,1), B, L_tot, F] indexed by t. */
int  cindm_ddpm1d_sample_guided(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                                const cindm_compose_desc* c, const cindm_design_desc* dz, float* x,
                                const float* cond, const float* noise_steps,
                                const float* recur_noise_steps, uint64_t seed, int64_t sample_offset,
                                const float* inpaint_cond, int32_t inpaint_steps,
                                const float* inpaint_noise_steps,
                                const float* initial_state_overwrite, int32_t overwrite_steps,
                                int32_t t_start, int32_t t_end, int64_t B,
                                void* ws, size_t ws_bytes, void* stream, int32_t use_graph);

/* DDIM loop (ddim_sample, model/diffusion_1d.py:1724-1804, design_fn == None): n_steps updates
 * x <- x0 * sqrt(alpha_next) + c * eps + sigma * z at times[0] > times[1] > ... > times[n_steps]
 * (times[n_steps] == -1: the last update returns x0); times [n_steps + 1] and coefs [n_steps][3] =
 * (sqrt(alpha_next), c, sigma) are HOST arrays computed by the caller in the reference's tensor
 * arithmetic (:1743-1777).  x0 is clamped when c->clip_denoised, eps is the model's (composed)
 * prediction, not re-derived (:1755).  noise_steps / inpaint_noise_steps, when given, are indexed
 * by the STEP index: [n_steps, B, L, F] / [n_steps, B, inpaint_steps, F]. */
int  cindm_ddpm1d_sample_ddim(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                              const cindm_compose_desc* c, float* x, const float* cond,
                              int32_t n_steps, const int32_t* times, const float* coefs,
                              const float* noise_steps, uint64_t seed, int64_t sample_offset,
                              const float* inpaint_cond, int32_t inpaint_steps,
                              const float* inpaint_noise_steps, int64_t B,
                              void* ws, size_t ws_bytes, void* stream, int32_t use_graph);

/* Guided DDIM loop (ddim_sample :1724-1804 with design_fn = the built-in objective and "standard" / "standard-alpha"
 * "-recurrence-N" guidance, N = dz->recurrence >= 1; every step goes through the DDIM return of p_sample_compose_inside,
 * :1284-1376).  Per DDIM step i, (t, t_next) = (times[i], times[i+1]), on the state x [B, L_tot, F]:
 *   y = x; for r = 0 .. N-1: (mean, x_start, eps) = p_mean_variance(y, t) under c (the compose descriptor IS honoured here,
 *   unlike cindm_ddpm1d_sample_ddim; x_start clamped when c->clip_denoised -- the reference always clamps on this path);
 *   g = [eta_t] grad objective(y), eta_t = betas[t] / sqrt(alphas_cumprod_prev[t]) when dz->alpha;
 *   pred = mean - g, rows < overwrite_steps replaced by initial_state_overwrite [B, overwrite_steps, F] if given;
 *   y = sqrt(abar_t/abar_{t-1}) pred + sqrt(1 - abar_t/abar_{t-1}) z'_{i,r}        (not computed for r = N-1: never used);
 *   x = x_start * sqrt(alpha_next) + c * (eps + g) + sigma * z_i with (x_start, eps, g) of iteration N-1, each product and
 *   sum rounded once; x = x_start when t_next < 0; otherwise, when inpaint_cond is given,
 *   x[:, :inpaint_steps] = q_sample(inpaint_cond, t, z^c_i).
 * times / coefs as cindm_ddpm1d_sample_ddim.  Tapes, when given, are indexed by the STEP index: noise_steps [n_steps, B, L_tot, F],
 * recur_noise_steps [n_steps, N, B, L_tot, F], inpaint_noise_steps [n_steps, B, inpaint_steps, F].  Without them the draws are
 * the counter-based Gaussians of cindm_ddpm1d_sample_guided (relaxation r of timestep t) and cindm_ddpm1d_sample_ddim (step and
 * inpainting draws), keyed by (seed, sample_offset + b, t, element): a design's result does not depend on the batch partition.
 * One relaxation iteration = the U-Net launches + one update launch: the state alternates between x and a slice of ws, the step
 * state between its two device slots, both advanced by the update itself (no copy, no counter launch in the captured step; two
 * DDIM steps per graph).  A chain like the others (recovery, range rule, graph cache, use_graph = 0 streams the same launches);
 * ws as cindm_ddpm1d_sample (cindm_ddpm1d_workspace_bytes for c already holds the second state buffer). */
int  cindm_ddpm1d_sample_ddim_guided(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                                     const cindm_compose_desc* c, const cindm_design_desc* dz, float* x,
                                     const float* cond, int32_t n_steps, const int32_t* times, const float* coefs,
                                     const float* noise_steps, const float* recur_noise_steps, uint64_t seed,
                                     int64_t sample_offset, const float* inpaint_cond, int32_t inpaint_steps,
                                     const float* inpaint_noise_steps, const float* initial_state_overwrite,
                                     int32_t overwrite_steps, int64_t B, void* ws, size_t ws_bytes, void* stream,
                                     int32_t use_graph);

/* Autoregressive time composition (autoregress_time_compose_sample, model/diffusion_1d.py:2240-2327):
 * n_seg segments of the unguided DDIM loop above, each on a fresh x_T [B, R, F] (R = the state length
 * the descriptor implies, c->cond_steps = Lc >= 1, R >= Lc) and conditioned on cond_buf [B, Lc, F]:
 * segment 0 on the caller's cond [B, Lc, F], segment k > 0 on the last Lc rows of segment k-1.
 * Segment k's final state goes to out[:, k*R : (k+1)*R] of out [B, n_seg*R, F].  x [B, R, F] and
 * cond_buf are caller-owned scratch (x holds the last segment's state on return); x, cond_buf, out and
 * init_tape must be 16-byte aligned.  times / coefs as cindm_ddpm1d_sample_ddim, shared by every
 * segment; seeds is a HOST array [n_seg]: segment k's x_T is the cindm_fill_normal draw (seeds[k],
 * sample_offset + b, step_tag = timesteps) and its step noise is keyed by seeds[k] as in
 * cindm_ddpm1d_sample_ddim -- so segment k computes what cindm_ddpm1d_sample_ddim(seed = seeds[k])
 * computes on its condition.  init_tape [n_seg, B, R, F] and noise_steps [n_seg, n_steps, B, R, F],
 * when given, replace those draws.  One chain for the recovery (a time-out re-runs the whole rollout
 * once, exchange-free) and one captured step graph for every segment when use_graph. */
int  cindm_ddpm1d_sample_autoregress(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                                     const cindm_compose_desc* c, float* x, const float* cond,
                                     float* cond_buf, float* out, int32_t n_seg, int32_t n_steps,
                                     const int32_t* times, const float* coefs, const uint64_t* seeds,
                                     const float* init_tape, const float* noise_steps,
                                     int64_t sample_offset, int64_t B, void* ws, size_t ws_bytes,
                                     void* stream, int32_t use_graph);

/* Parallel time composition (composing_time_sample, model/diffusion_1d.py:1807-1854; the "EBMs_compose" method of
 * inference/inference_1d_composing_time_steps.py:171-178): ONE unguided DDIM chain on the n_seg * B rows of x [n_seg * B, R, F],
 * segment-major (row k * B + b), R = the state length the descriptor implies, c->cond_steps = Lc >= 1, R >= Lc, n_seg >= 2,
 * n_seg * B <= 65535; plain or multibody prediction, as cindm_ddpm1d_sample_autoregress.  Per DDIM step i,
 * (t, t_next) = (times[i], times[i+1]):
 *   cond_buf[(k+1) * B + b] = x[k * B + b, R - Lc : R]  for k = 0 .. n_seg - 2: the CURRENT, still noisy state (:1827-1829);
 *   rows 0 .. B of cond_buf [n_seg * B, Lc, F] hold the caller's cond [B, Lc, F] and never change;
 *   (eps, x_start) = model_predictions(x, cond_buf, t): one U-Net evaluation on all n_seg * B rows of cat(cond_buf, x), x_start
 *   clamped when c->clip_denoised, eps the model's prediction, not re-derived (:1838);
 *   x = x_start * sqrt(alpha_next) + c * eps + sigma * z_i, each product and sum rounded once; x = x_start when t_next < 0.
 * So the chain takes n_steps sequential steps where the autoregressive rollout takes n_seg * n_steps, and segments k >= 1 see a
 * noisy condition throughout: a different algorithm, not a faster form of the rollout.  On return x holds all n_seg final states
 * (the caller assembles the reference's (img, img_infered) pair from it) and cond_buf the last hand-over.
 * times / coefs as cindm_ddpm1d_sample_ddim.  seeds is a HOST array [n_seg]: segment k's x_T is the cindm_fill_normal draw
 * (seeds[k], sample_offset + b, step_tag = timesteps) and the step noise of row (k, b) is keyed (seeds[k], sample_offset + b, t,
 * element of [R, F]) -- the rule of cindm_ddpm1d_sample_autoregress, so a design's result depends neither on B nor on how a batch
 * is partitioned, and segment 0 computes what cindm_ddpm1d_sample_ddim(seed = seeds[0]) computes on cond.  init_tape
 * [n_seg, B, R, F] and noise_steps [n_steps, n_seg, B, R, F] (indexed by the STEP index, read whenever t_next >= 0), when given,
 * replace those draws.  x, cond, cond_buf and the tapes must be 16-byte aligned (the update moves 16 bytes per lane).
 * One launch per step does the update AND the hand-over (timecompose_update_kernel: a thread that writes a tail row of segment
 * k < n_seg - 1 also writes it into cond_buf of segment k + 1; the step's U-Net input was gathered from cond_buf before that
 * launch); one more launch before the first step draws x_T, hands over from it and copies cond.  A chain like the others: one
 * captured step graph, replayed (use_graph = 0 streams the same launches); an exchange time-out re-runs the whole chain once on
 * the exchange-free kernels; the range rule applies; cindm_ddpm1d_last_chain_info answers for it; cindm_ddpm1d_set_recorder is
 * served with a record of [n_seg * B, R, F] per step i = 0 .. n_steps - 1 (both streams).  An armed known region or armed design
 * tables are refused.  ws as cindm_ddpm1d_sample with cindm_ddpm1d_workspace_bytes(h, pair, uncond, c, n_seg * B): nothing is
 * allocated (the segment seeds are kept in the workspace's second state buffer). */
int  cindm_ddpm1d_sample_timecompose(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                                     const cindm_compose_desc* c, float* x, const float* cond,
                                     float* cond_buf, int32_t n_seg, int32_t n_steps,
                                     const int32_t* times, const float* coefs, const uint64_t* seeds,
                                     const float* init_tape, const float* noise_steps,
                                     int64_t sample_offset, int64_t B, void* ws, size_t ws_bytes,
                                     void* stream, int32_t use_graph);

/* Langevin (ULA) phase of sample_compose_multibodies (model/diffusion_1d.py:2002-2022 -> sample_step_ULA :2048-2073 on the
 * composed score of gradient() :1865-1926): for t = t_start, t_start-1, ..., t_end, L times
 *   eps = composed noise of gradient(x, t)       (CINDM_COMPOSE_MULTIBODY with c->uncond_coef; both U-Nets see timestep t)
 *   x   = (x + (fl(-scalar_t) * eps) * fl(ss_t)) + z * fl(std_t)      (:1924, :2056, :2059, each product and sum rounded once)
 * in place on x [B, L_tot, F], which is the WHOLE state cat(cond, x) of the reference (:1988): c->cond_steps must be 0 and
 * L_tot = the models' horizon, so the conditioning rows are rows of x and move too.  c->objective must be CINDM_OBJ_PRED_NOISE,
 * c->clip_denoised is not used.  That the reference only runs this above t = 400 is the caller's business: any range inside
 * [0, timesteps) is accepted.  L == 0 returns at once.
 * scalar / step_size / noise_std: HOST arrays [t_start - t_end + 1], entry j for timestep t_start - j, computed by the caller
 * in the reference's fp64 tensor arithmetic and cast to fp32 (scalar_t = sqrt(1 / (1 - cumprod(1 - betas_inference)_t)) :1998-1999,
 * ss_t = betas_inference_t * 0.035 :2050, std_t = (2 ss_t) ** .5 :2054); the library copies them to tab, a caller-owned DEVICE
 * buffer of at least (t_start - t_end + 1) * 16 bytes, 16-byte aligned, that must stay alive until the call's work has finished.
 * noise_tape: NULL or a device tensor [t_start - t_end + 1, L, B, L_tot, F] in processing order (row j of the first axis is
 * timestep t_start - j), 16-byte aligned like x.  Without it z is the counter-based Gaussian keyed by
 * (seed, sample_offset + b, step word 0x80000000 + l * 65536 + t, element of [L_tot, F]) for inner iteration l of timestep t
 * (L <= 32767, timesteps <= 65536): the step words of x_T (= timesteps) and of the DDPM / DDIM steps (= t) are below 2^31, so
 * the draws are disjoint from theirs, and they depend neither on B nor on how a range of timesteps is split over calls.
 * One captured HIP graph per Langevin iteration (gather, both U-Nets, one element-wise update), replayed
 * (t_start - t_end + 1) * L times when use_graph; the timestep and the inner index live in device memory and advance there (the
 * timestep once per L replays).  A chain like the others: exchange time-outs are read at its end and the chain is re-run once
 * from its initial x on the exchange-free kernels; cindm_ddpm1d_last_chain_info answers for it.  ws as cindm_ddpm1d_sample
 * (cindm_ddpm1d_workspace_bytes for c). */
int  cindm_ddpm1d_sample_ula(cindm_ddpm1d* h, cindm_unet1d* pair, cindm_unet1d* uncond,
                             const cindm_compose_desc* c, float* x, int32_t t_start, int32_t t_end, int32_t L,
                             const float* scalar, const float* step_size, const float* noise_std,
                             void* tab, size_t tab_bytes, const float* noise_tape, uint64_t seed,
                             int64_t sample_offset, int64_t B, void* ws, size_t ws_bytes, void* stream,
                             int32_t use_graph);

/* out[n] ~ N(0,1): the library's counter-based Gaussian (Philox4x32-10 + Box-Muller) for the
 * initial state x_T (:1673), keyed by (seed, sample_offset + b, step_tag, element);
 * out is [B, per_sample]. */
int  cindm_fill_normal(float* out, int64_t B, int64_t per_sample, uint64_t seed,
                       int64_t sample_offset, int32_t step_tag, void* stream);

/* Timing aid for bench.py: elapsed ms of `n_replays` steps measured with HIP events on `stream`
 * is done by the caller; this returns the number of kernel launches in one step. */
int  cindm_ddpm1d_launches_per_step(const cindm_ddpm1d* h, const cindm_unet1d* pair,
                                    const cindm_unet1d* uncond, const cindm_compose_desc* c);

/* What the reverse step emitted LAST on this handle consisted of (by cindm_ddpm1d_step / _predict or by the
 * capture of a sample loop): `launches` = kernels launched (gather + U-Net(s) + update + step counter), as
 * launched, not modelled; `fused_update` = 1 when the reverse-step update (:1033-1044, :1281) ran inside the
 * U-Net's last kernel instead of compose_update_kernel.  Tests assert the fused path through this. */
int  cindm_ddpm1d_last_step_info(const cindm_ddpm1d* h, int32_t* launches, int32_t* fused_update);
/* What the last sampling chain of this handle did: info[0] = 1 when it was re-run once on the exchange-free plan after an in-kernel
 * exchange timed out; info[1] = 1 when it ran on the exchange-free plan from the start because another chain was already in flight
 * on the device in this process (one chain per device is the rule of the exchange kernels; the registry is per process);
 * info[2] = chains in flight on the device when it started, itself included.  No reference counterpart. */
int  cindm_ddpm1d_last_chain_info(const cindm_ddpm1d* h, int32_t info[4]);

/* The chain recorder: every `every`-th state of a sampling chain, copied by one more kernel of the captured step
 * (chain_record_kernel).  No reference counterpart (its scripts collect per-step lists from inside their Python loops).
 * cindm_ddpm1d_set_recorder arms the NEXT chain call on this handle; that call consumes the recorder whether it succeeds or fails,
 * and buf == NULL disarms.  A chain runs n steps i = 0 .. n-1 (DDPM: n = t_start - t_end + 1, step i is timestep t_start - i; DDIM:
 * n = n_steps, step i is times[i]; a guided step with relaxation iterations is ONE step).  The state after step i is recorded iff
 * (i + 1) % every == 0 or i == n - 1: ceil(n / every) records, the last one is the chain's result.
 * streams: bit 0 = x, the state the step leaves behind; bit 1 = x0, the x_start the step predicted, clamped as its update used it
 * (a guided step: that of its last iteration).  Any other bit, every < 1 or an unaligned buffer is refused here.
 * buf: DEVICE memory, 16-byte aligned, buf_floats floats, laid out as [records][streams, x before x0][floats per record], followed
 * by ONE more record when x0 is on (the update kernel stages its x_start there).  A record is the chain's state in the library's
 * own layout: [B, L_tot, F] for the 1-D entries, [B * nb, H * W, padded channels] for the 2-D entries.  The chain call refuses a
 * buffer that is too small for it, or a state x that is not 16-byte aligned, before it launches or copies anything (x is untouched).
 * An every above the chain's step count records what every == steps records: the result alone.  Record offsets are 64-bit.
 * Served by cindm_ddpm1d_sample / _sample_guided / _sample_ddim / _sample_ddim_guided and cindm_ddpm2d_sample / _sample_ddim /
 * _sample_force / _sample_ddim_force (x0: not by the two 2-D DDIM entries, whose update kernels have no x0 operand); refused by
 * cindm_ddpm1d_sample_autoregress and _sample_ula.  A chain that is re-run on the exchange-free plan records again from record 0.
 * With no recorder armed a chain launches exactly what it launched before this entry existed; with one, one launch more per step
 * (and a plain 1-D step runs compose_update_kernel instead of the update fused into the U-Net's last kernel when x0 is on).
 * cindm_ddpm1d_recorder_info: info[0] = records the last chain call wrote (0: it had no recorder, or failed), info[1] = floats
 * per record, info[2] = steps run, info[3] = streams. */
int  cindm_ddpm1d_set_recorder(cindm_ddpm1d* h, float* buf, int64_t buf_floats, int32_t every, int32_t streams);
int  cindm_ddpm1d_recorder_info(const cindm_ddpm1d* h, int32_t info[4]);

/* The waypoint objective's tables (cindm_design_desc modes 3 / 4).  No reference counterpart: its script evaluates one target
 * per sample() call (inference/inverse_design_diffusion_1d.py:283-315); here a batch can carry a target and a weight per design.
 * target: DEVICE floats [batch, rows, n_bodies, 2] when target_per_design, else [rows, n_bodies, 2] shared by every design: the
 * position (features 4j, 4j+1) body j is drawn to at that row, in state units.
 * scale:  DEVICE floats [batch, rows, n_bodies] when scale_per_design, else [rows, n_bodies]: finite and >= 0; an entry that is 0
 * contributes nothing to the gradient (its target is not read).  The update kernel evaluates, per position component,
 *   "L2": scale * d / sqrtf(d * d + d_other * d_other),  "L2square": scale * 2 * d,  d = pos - target,
 * the point objective's expressions with scale in place of coef / last_n_step.
 * cindm_ddpm1d_set_design_tables arms the NEXT chain call on this handle; that call consumes the tables whether it succeeds or
 * fails, and (NULL, NULL) disarms.  cindm_ddpm1d_sample_guided / _sample_ddim_guided check rows == L_tot, n_bodies == c->n_bodies,
 * batch == B and that both tables are 16-byte aligned before they launch or copy anything, and refuse modes 3 / 4 with nothing
 * armed and armed tables with modes 1 / 2; every other chain entry, 1-D or 2-D, refuses armed tables.  The tables must stay alive and
 * unchanged until the chain's work has finished: with use_graph that is when the call returns (it synchronises; an exchange-free
 * re-run inside the call reads them again); with use_graph = 0 the steps are only enqueued on the caller's stream, so the tables
 * must outlive that stream's work (free or overwrite them after a synchronise, or in stream order).  Their addresses and the two
 * flags are operands of the captured update: a call with other tables captures its step again. */
int  cindm_ddpm1d_set_design_tables(cindm_ddpm1d* h, const float* target, int32_t target_per_design,
                                    const float* scale, int32_t scale_per_design,
                                    int32_t rows, int32_t n_bodies, int64_t batch);

/* The quadratic objective's tables (cindm_design_desc mode 5).  No reference counterpart.  Everything that is linear-quadratic in the
 * features of one row -- a velocity target, a relation between bodies, the centre of mass or the total momentum at a row, any weighted
 * least-squares mix of such terms -- is one (S, h) pair per row; the gradient acts on all four components of a body.
 * S:    DEVICE floats [batch, rows, features, features] when S_per_design, else [rows, features, features] shared by every design;
 *       every S[.., l] symmetric.  features = 4 * n_bodies, a multiple of 4 in 4 .. 32.
 * hvec: DEVICE floats [batch, rows, features] when h_per_design, else [rows, features].
 * The update kernel (compose_update_quad_kernel, the guided update compiled with this gradient) evaluates at element (b, l, f)
 *   g = (sum_{f' = 0 .. features - 1} S[l, f, f'] * x[b, l, f']) - hvec[l, f]
 * from 0.f in ascending f', every product and every sum rounded once to fp32 (no contraction), the subtraction last; then the
 * time-consistency term on the position features, the standard-alpha factor and the rest of the guided update as for modes 1 - 4.
 * cindm_ddpm1d_set_design_quadratic arms the NEXT chain call on this handle; that call consumes the tables whether it succeeds or
 * fails, and (NULL, NULL) disarms.  cindm_ddpm1d_sample_guided / _sample_ddim_guided check rows == L_tot, features == 4 * c->n_bodies,
 * batch == B and that S, hvec and the state x are 16-byte aligned (rows of S and of x are read 16 bytes at a time) before they launch
 * or copy anything.  They refuse mode 5 with nothing armed, armed quadratic tables with modes 1 - 4, and the tables of
 * cindm_ddpm1d_set_design_tables with mode 5; every other chain entry -- the unguided 1-D chains, the rollout, the time composition,
 * the Langevin chain and all 2-D chains -- refuses armed quadratic tables and says why.  Lifetime as for the waypoint tables: they
 * must stay alive and unchanged until the chain's work has finished -- with use_graph that is when the call returns (it
 * synchronises; an exchange-free re-run inside the call reads them again); with use_graph = 0 the steps are only enqueued on the
 * caller's stream, so the tables must outlive that stream's work (free or overwrite them after a synchronise, or in stream order).
 * The two addresses and the two flags are operands of the captured update: a call with other tables captures its step again. */
int  cindm_ddpm1d_set_design_quadratic(cindm_ddpm1d* h, const float* S, int32_t S_per_design,
                                       const float* hvec, int32_t h_per_design,
                                       int32_t rows, int32_t features, int64_t batch);

/* The pair-distance objective's tables (cindm_design_desc mode 6).  No reference counterpart.  A relation between the positions of two
 * bodies that is not quadratic -- "stay at least d apart" (lo = d, hi = +inf), "come within d" (lo = 0, hi = d), "meet at distance d"
 * (lo = hi = d) -- is one (lo, hi, weight) entry per (design | all designs, row, pair); relations mix freely in one table.
 * Pairs p = (i, j), i < j, are ordered (0,1), (0,2), .., (1,2), ..: p = i * n_bodies - i (i + 1) / 2 + (j - i - 1); P = n_bodies (n_bodies - 1) / 2.
 * band:   DEVICE floats [batch, rows, P, 2] when band_per_design, else [rows, P, 2] shared by every design: (lo, hi) interleaved,
 *         0 <= lo <= hi, lo finite, hi finite or +inf.
 * weight: DEVICE floats [batch, rows, P] when weight_per_design, else [rows, P]; finite, >= 0.
 * The update kernel (compose_update_pair_kernel, the guided update compiled with this gradient) evaluates at the position component
 * c (0: x, 1: y) of body i at (b, l), from g = 0.f over the other bodies o in ascending o, g = g + term(i, o):
 *   d  = x[b, l, 4 i + c] - x[b, l, 4 o + c],   d' = the same difference of the other position component,
 *   r  = sqrt(d * d + d' * d'),
 *   term = ((((w * 2) * (r - lo)) * d) / r  where r < lo,   ((((w * 2) * (r - hi)) * d) / r  where r > hi,   0.f otherwise,
 * and 0.f where w == 0 or r == 0 (w, lo, hi: the entry of the pair {i, o}); every difference, product, sum, square root and quotient
 * is rounded once to fp32 (no contraction), in the order written.  Velocity components get no term.  Then the time-consistency term,
 * the standard-alpha factor and the rest of the guided update as for modes 1 - 5.  The gradient reads the element's own row of x only.
 * cindm_ddpm1d_set_design_pairdist arms the NEXT chain call on this handle (n_bodies in 2 .. 8); that call consumes the tables whether
 * it succeeds or fails, and (NULL, NULL) disarms.  cindm_ddpm1d_sample_guided / _sample_ddim_guided check rows == L_tot, n_bodies ==
 * c->n_bodies and batch == B before they launch or copy anything, under every compose mode they serve, and _sample_ddim_guided also
 * with the multistep solver armed (compose_update_pair_kernel<true>).  They refuse mode 6 with nothing armed, armed pair-distance tables
 * with modes 1 - 5, and the tables of cindm_ddpm1d_set_design_tables or cindm_ddpm1d_set_design_quadratic with mode 6; every other
 * chain entry -- the unguided 1-D chains, the rollout, the time composition, the Langevin chain and all 2-D chains -- refuses armed
 * pair-distance tables and says why.  A refusal leaves the handle usable.  Lifetime and capture as for the quadratic tables: caller-owned,
 * alive and unchanged until the chain's work has finished; the two addresses and the two flags are operands of the captured update, so
 * a call with other tables captures its step again.  The workspace size does not change. */
int  cindm_ddpm1d_set_design_pairdist(cindm_ddpm1d* h, const float* band, int32_t band_per_design,
                                      const float* weight, int32_t weight_per_design,
                                      int32_t rows, int32_t n_bodies, int64_t batch);

/* Replacement conditioning of the 2-D chains: a known region of the state [B * nb, H * W, CP] is held on the forward-diffusion
 * trajectory of its clean values and returned exactly (known2d_kernel: one more node of the captured step, after the step's
 * update, guidance shift and counter).  No reference counterpart: its 2-D sample() takes no condition; the 1-D entries keep the
 * reference's inpainting through their own arguments.  With q(k, t, z) = sqrt_alphas_cumprod[t] k + sqrt_one_minus_alphas_cumprod[t] z
 * (two products and a sum, each rounded once):
 *   before the first step, which is at timestep t0:   x[m] = q(k, t0, z_init)
 *   after a step from t to t_next (DDPM: t - 1, DDIM: times[i + 1]):   x[m] = q(k, t_next, z) if t_next >= 0, else x[m] = k
 * so the chain's result carries k exactly on the region (a DDPM chain with t_end > 0 ends at level t_end - 1 like the rest of its
 * state).  z is drawn like the step noise -- state channels (all but the last 3) once per design, shared by its nb images, boundary
 * channels per image -- at every step, whatever the DDIM sigma.
 * known: DEVICE floats [images, hw, cp], the clean values (read only where the mask is set).
 * mask:  DEVICE bytes [images, hw, cp / 4]: bit j of a byte = channel 4 g + j of that image and pixel is known; bits of padded
 *        channels are ignored (padding stays zero).  The state channels of known and mask must be the same for the nb images of
 *        a design (the caller's duty; otherwise the chains lose their invariant that those channels are shared).
 * noise_init_state [B, hw, C-3], noise_init_boundary [images, hw, 3], noise_state_steps [rows][B, hw, C-3], noise_boundary_steps
 *        [rows][images, hw, 3] with the two row strides in floats: explicit z for parity runs, all four or none; row = t (DDPM) or
 *        the DDIM step index, as the chains' own step tapes.  None: the counter-based generator under a seed word of its own, keyed
 *        (seed, sample_offset + design, t_next) with the chain call's seed and sample_offset; z_init is keyed by the timestep count.
 * cindm_ddpm1d_set_known2d arms the NEXT chain call on this handle; that call consumes the region whether it succeeds or fails, and
 * (NULL, NULL) disarms.  Served by cindm_ddpm2d_sample / _sample_ddim / _sample_force / _sample_ddim_force, which check images ==
 * B * nb, hw == H * W, cp == CP, the strides and the 16-byte alignment of x before they launch or copy anything; every 1-D chain
 * entry refuses an armed region.  All buffers are the caller's, 16-byte aligned, and must stay alive and unchanged until the chain's
 * work has finished (use_graph: when the call returns; otherwise in stream order).  Their addresses are operands of the captured node.
 * An exchange-free re-run starts from the first rule again; a recorder records after the overwrite.  With nothing armed a chain
 * launches exactly what it launched before this entry existed; with a region, one launch more per step and one per chain. */
int  cindm_ddpm1d_set_known2d(cindm_ddpm1d* h, const float* known, const uint8_t* mask,
                              const float* noise_init_state, const float* noise_init_boundary,
                              const float* noise_state_steps, const float* noise_boundary_steps,
                              int64_t state_step_stride, int64_t boundary_step_stride,
                              int64_t images, int32_t hw, int32_t cp);

/* Replacement conditioning of the 1-D chains: a known region of the state x [B, rows, F] (the rows sample() returns; F = 4 * n_bodies)
 * is held on the forward-diffusion trajectory of its clean values k and returned exactly (known1d_kernel: one more node of the
 * captured step, after the update in whichever form -- fused into the U-Net's last kernel, compose_update_kernel, guided -- after the
 * guided DDPM step's staging copy and the counter, before the record node).  No reference counterpart; inpaint_cond and
 * initial_state_overwrite keep the reference's semantics.  With q(k, l, z) = sqrt_alphas_cumprod[l] k + sqrt_one_minus_alphas_cumprod[l] z
 * (two products and a sum, each rounded once):
 *   before the first step, which is at timestep t0 (apply_init != 0):   x[m] = q(k, t0, z_init)
 *   after relaxation iteration r of a guided step at t (the state is back at level t):   x[m] = q(k, t, z)
 *   after the step's last update, t -> t_next (DDPM: t - 1, DDIM: times[i + 1]):   x[m] = q(k, t_next, z) if t_next >= 0, else x[m] = k
 * so the chain's result carries k exactly on the region (a DDPM chain with t_end > 0 ends at level t_end - 1 like the rest).  The
 * level is read from the device step state, so one captured graph serves every step.  The region overwrites last: rows also claimed
 * by inpaint_cond or initial_state_overwrite carry the region's values.
 * known: DEVICE floats [batch | 1, rows, feats] (known_per_design != 0: one table per design; 0: one shared by all designs).
 * mask:  DEVICE bytes of the same layout, [batch | 1, rows, feats] by mask_per_design: non-zero = the element is known.
 * noise_init [batch, rows, feats]; noise_steps [.][batch, rows, feats] with step_stride floats between rows, row = t (DDPM) or the
 *        DDIM step index, as the chains' own step tapes; noise_recur [.][iters][batch, rows, feats] with recur_stride floats between
 *        rows, record r read after relaxation r (iters = the guided step's iterations, as the chains' recurrence tape): explicit z
 *        for parity runs.  noise_steps NULL (then all three NULL): the counter-based generator under a seed word of its own, keyed
 *        (seed, sample_offset + design, word, element) with the chain call's seed and sample_offset; word = t_next after a step,
 *        t + 0x10000 (r + 1) after relaxation r, the timestep count for z_init.  noise_recur is needed only by a guided chain with more
 *        than one iteration per step; noise_init only with apply_init.
 * apply_init: 0 skips the first rule -- for a caller that hands over a state already at its level (teacher-forced DDIM segments).
 * cindm_ddpm1d_set_known1d arms the NEXT chain call on this handle; that call consumes the region whether it succeeds or fails, and
 * (NULL, NULL) disarms.  Served by cindm_ddpm1d_sample / _sample_guided / _sample_ddim / _sample_ddim_guided, which check batch == B,
 * rows and feats against the state, the strides and the 16-byte alignment of x and of the workspace's second state buffer before they
 * launch or copy anything; cindm_ddpm1d_sample_autoregress, cindm_ddpm1d_sample_ula and every 2-D chain entry refuse an armed region.
 * All buffers are the caller's, 16-byte aligned, and must stay alive and unchanged until the chain's work has finished (use_graph:
 * when the call returns; otherwise in stream order).  Their addresses are operands of the captured node and part of the graph's key.
 * An exchange-free re-run starts from the first rule again; a recorder records x after the overwrite, x0 is the model's prediction.
 * With nothing armed a chain launches exactly what it launched before this entry existed (the same cindm_ddpm1d_last_step_info
 * count, the same graph key); with a region, one launch more per update and one per chain. */
int  cindm_ddpm1d_set_known1d(cindm_ddpm1d* h, const float* known, int32_t known_per_design,
                              const uint8_t* mask, int32_t mask_per_design,
                              const float* noise_init, const float* noise_steps, int64_t step_stride,
                              const float* noise_recur, int64_t recur_stride, int32_t apply_init,
                              int64_t batch, int32_t rows, int32_t feats);

/* Second-order multistep solver on the DDIM chains (DPM-Solver++ 2M in data-prediction form).  For the pair (X, E) a
 * chain hands to its DDIM update -- x' = sqrt(alpha_next) X + c E (+ sigma z, which the solver requires to be 0) -- step i computes
 *     x' = [that DDIM value] + kappa[i] * (X_i - X_{i-1}),
 * the difference, the product and the sum rounded once each, ahead of whatever follows the DDIM value today (the 2-D guidance shift,
 * the inpainting overwrite, the known-region node, the recorder), and writes X_i to hist.  A step with kappa[i] == 0 does not read
 * hist -- the first step of a chain needs no initialised history -- and the last pair (time_next < 0) returns X as before.  In a
 * guided 1-D step only the iteration that performs the DDIM update reads and writes hist; relaxation iterations leave it alone.
 * kappa_host: HOST floats [n_steps], copied by this call (schedule.multistep_kappa of the Python face computes them in float64:
 *        kappa_i = (alpha' - sigma' alpha / sigma) h_i / (2 h_{i-1}) with lambda = ln(alpha / sigma), h_i = lambda' - lambda, kappa_0 = 0;
 *        a caller that continues a chain passes kappa_0 != 0 and the history X_{-1} in hist).
 * hist:  DEVICE floats shaped like the chain's state (1-D: [B, L_tot, F]; 2-D: the channel-last padded layout of x), 16-byte
 *        aligned, the caller's, distinct from the state; hist_floats: its length, which must equal the state's.  On return it holds
 *        the X of the last step.
 * Arms the NEXT chain call on this handle; that call consumes the solver whether it succeeds or fails, and kappa_host == NULL
 * disarms.  Run by cindm_ddpm1d_sample_ddim / _sample_ddim_guided and cindm_ddpm2d_sample_ddim / _sample_ddim_force, which check
 * n_steps against the call, hist_floats against the state and that every step's sigma is 0; every other chain entry refuses an armed
 * solver.  The 2-D entries keep kappa behind their tables: tab_bytes must then be >= n_steps * 24.  cindm_ddpm1d_workspace_bytes is
 * unchanged.  The multistep 1-D step never runs its update inside the last U-Net kernel (one launch more than the fused DDIM step).
 * A chain whose first step reads the history (kappa[0] != 0) cannot be re-run after an exchange time-out: the call fails and says so.
 * With nothing armed a chain launches exactly what it launched before this entry existed, under the same graph key. */
int  cindm_ddpm1d_set_multistep(cindm_ddpm1d* h, const float* kappa_host, int32_t n_steps, float* hist, int64_t hist_floats);

/* ===================================================================== 2-D airfoil path
 * Replaces Unet.forward (model/diffusion_2d.py:369-408) and GaussianDiffusion.p_sample /
 * p_sample_loop (model/diffusion_2d.py:788-907) of the reference for the sampling path
 * (no self-conditioning, no learned variance, objective pred_noise).
 *
 * Device layout of states and model outputs: channel-last fp32 [images, H*W, CP] with
 * CP = cindm_unet2d_padded_channels() (channels rounded up to a multiple of 4; padding
 * channels are zero).  An "image" is one boundary of one design: images = B * num_boundaries,
 * boundary-major inside a design, exactly the reference's [B, nb*C, H, W] -> [B*nb, C, H, W]
 * view (:901). */
typedef struct cindm_unet2d cindm_unet2d;

typedef struct {
    int32_t dim;              /* Unet(dim=...)                              :283 */
    int32_t n_mults;
    int32_t dim_mults[4];     /* entries 1 or 2                             :287 */
    int32_t channels;         /* 21 for the airfoil states (6 frames*3 + 3) :288 */
    int32_t image_size;       /* square, power of two <= 64                 :660 */
    int32_t timesteps;        /* rows of the per-timestep scale/shift table */
} cindm_unet2d_desc;

int  cindm_unet2d_create(const cindm_unet2d_desc* desc, cindm_unet2d** out);
void cindm_unet2d_destroy(cindm_unet2d* h);
int  cindm_unet2d_num_params(const cindm_unet2d* h);
int  cindm_unet2d_param_info(const cindm_unet2d* h, int idx, char* name, int name_cap,
                             int64_t shape[4], int* ndim);
int  cindm_unet2d_set_param(cindm_unet2d* h, const char* key, const float* src, int64_t numel,
                            int on_device);
int  cindm_unet2d_set_sinusoid_table(cindm_unet2d* h, const float* table, int64_t numel);
/* Weight standardisation (WeightStandardizedConv2d :116-124) folded, MFMA-fragment repack,
 * time path (SinusoidalPosEmb -> Linear -> GELU -> Linear -> per block SiLU -> Linear, :320-326,
 * :205-208) evaluated for every timestep into a device table. */
/* Kernel-path selection, as cindm_unet1d_set_option (every key a pack option).  Keys: "mfma_f32", "la_site", "conv_ws" (1 = persistent
 * wave-specialised 3x3 kernel, 0 = per-tile kernel, 2 / 3 = only the plain-source / GroupNorm-on-load convolutions on
 * it), "ws_nosplit" (0 / 1 / 2: where that kernel splits K over its matrix waves), "tail_h3" (ResnetBlock tails with a res_conv GEMM
 * on the split-fp16 products), "ws_alias" (block-internal temporaries share workspace), "la_wpi" / "la_nsplit" (workgroups per image of
 * the LinearAttention kernels), "stress", "auto_range", "range_fallback" (read-only), "dbg2". */
int  cindm_unet2d_set_option(cindm_unet2d* h, const char* key, int32_t value);
int  cindm_unet2d_get_option(const cindm_unet2d* h, const char* key, int32_t* value);
int  cindm_unet2d_finalize(cindm_unet2d* h, void* stream);
int  cindm_unet2d_padded_channels(const cindm_unet2d* h);
size_t cindm_unet2d_workspace_bytes(const cindm_unet2d* h, int64_t images);
int  cindm_unet2d_launches_per_forward(const cindm_unet2d* h);
/* eps[images, H*W, CP] = Unet(x[images, H*W, CP], t); t_dev (device int32) wins over t. */
int  cindm_unet2d_forward(cindm_unet2d* h, const float* x, int32_t t, const int32_t* t_dev,
                          float* eps, int64_t images, void* ws, size_t ws_bytes, void* stream);
/* Measurement hook for bench.py: one forward with every launch bracketed by HIP events on
 * `stream`; per kernel kind (0 conv3x3, 1 conv1x1, 2 stem 7x7, 3 qkv 1x1, 4 linear attention,
 * 5 full attention, 6 statistics / LayerNorm-residual): launches, total ms, algorithmic FLOPs. */
int  cindm_unet2d_profile(cindm_unet2d* h, const float* x, int32_t t, float* eps, int64_t images,
                          void* ws, size_t ws_bytes, void* stream, int32_t counts[7], float ms[7],
                          double flops[7]);
/* Test hook: copy the intermediate activation `name` of the last forward into dst as
 * [images, H*W, C]; shape receives (images, H*W, C). */
int  cindm_unet2d_tap(cindm_unet2d* h, const char* name, int64_t images, void* ws, float* dst,
                      int64_t dst_cap, int64_t shape[3], void* stream);

size_t cindm_ddpm2d_workspace_bytes(const cindm_unet2d* u, int64_t images);
/* One reverse step x_t -> x_{t-1} of GaussianDiffusion.p_sample (:788-808) for B designs of
 * nb boundaries: Unet on all B*nb images; the model output's state channels (all but the last
 * 3) are averaged (use_average_share=1) or summed over the nb boundaries of a design
 * (share_states_over_boundaries :712-725); x0 from eps, clamp; posterior mean; + sigma_t * z
 * (use_average_share bit 1 set = the constructor's share_noise False, p_mean_variance :757-773: the
 * prediction is left alone and the clamped x_start, then the posterior mean, are shared instead)
 * with z shared over the boundaries for the state channels (sample_noise :775-785).  z comes
 * from noise_state [B, H*W, C-3] / noise_boundary [B*nb, H*W, 3] when given, else from the
 * counter-based generator (seed, sample_offset + b, t).  In place on x.  Optional outputs:
 * x0_out (clamped x_start), mean_out (posterior mean), both [B*nb, H*W, CP].
 * Bits 4-5 of use_average_share carry the diffusion's objective (CINDM_OBJ_*; :743-753): pred_x0 takes the model output as
 * x_start, pred_v takes x_start = sqrt(abar_t) x - sqrt(1 - abar_t) v; for both the reference shares nothing inside
 * model_predictions (share_noise False still shares x_start and the mean afterwards) and re-derives the noise from x_start.
 * The same word is used by cindm_ddpm2d_predict, cindm_ddpm2d_sample and cindm_ddpm2d_sample_force. */
int  cindm_ddpm2d_step(cindm_ddpm1d* sched, cindm_unet2d* u, float* x, int64_t B, int32_t nb,
                       int32_t use_average_share, int32_t clip_denoised,
                       const float* noise_state, const float* noise_boundary, uint64_t seed,
                       int64_t sample_offset, int32_t t, const int32_t* t_dev, float* x0_out,
                       float* mean_out, void* ws, size_t ws_bytes, void* stream);
/* GaussianDiffusion.model_predictions (:727-754; objective in bits 4-5 of use_average_share, see above) for B designs of nb boundaries: Unet on all
 * B*nb images; share_noise != 0: the model output's state channels are averaged (use_average_share = 1) or summed (0)
 * over the boundaries of a design (:732-733); x_start = predict_start_from_noise(x, t, pred_noise), clamped to [-1, 1]
 * when clip_x_start; rederive_pred_noise (with clip_x_start, :738-739): pred_noise = predict_noise_from_start(x, t,
 * x_start) = (sqrt_recip_t x - x_start) / sqrt_recipm1_t.  Writes pred_noise_out and x_start_out, both [B*nb, H*W, CP]
 * (either may be NULL); x is not modified. */
int  cindm_ddpm2d_predict(cindm_ddpm1d* sched, cindm_unet2d* u, const float* x, int64_t B, int32_t nb,
                          int32_t use_average_share, int32_t share_noise, int32_t clip_x_start,
                          int32_t rederive_pred_noise, int32_t t, const int32_t* t_dev,
                          float* pred_noise_out, float* x_start_out, void* ws, size_t ws_bytes, void* stream);
/* p_sample_loop (:893-907) without design guidance: steps t_start .. t_end in place on x, one
 * captured HIP graph replayed per step when use_graph.  noise_*_steps, when given, are indexed
 * [timesteps, ...] by t. */
int  cindm_ddpm2d_sample(cindm_ddpm1d* sched, cindm_unet2d* u, float* x, int64_t B, int32_t nb,
                         int32_t use_average_share, const float* noise_state_steps,
                         const float* noise_boundary_steps, uint64_t seed, int64_t sample_offset,
                         int32_t t_start, int32_t t_end, void* ws, size_t ws_bytes, void* stream,
                         int32_t use_graph);
/* DDIM loop of the 2-D path (GaussianDiffusion.ddim_sample, design_fn == None, share_noise True): n_steps updates
 * in place on x at times[0] > times[1] > ... > times[n_steps] >= -1, each
 *   (eps, x0) = model_predictions(x, t, clip_x_start=1, rederive_pred_noise=1, share_noise=1)   (:727-754)
 *   x = times[i+1] < 0 ? x0 : x0 * sqrt(alpha_next) + c * eps + sigma * z
 * with z shared over the boundaries for the state channels (sample_noise :775-785).  times [n_steps + 1]
 * and coefs [n_steps][3] = (sqrt(alpha_next), c, sigma) are HOST arrays computed by the caller (as for
 * cindm_ddpm1d_sample_ddim); the library copies them to tab, a caller-owned DEVICE buffer of at least
 * n_steps * 5 * 4 bytes, 16-byte aligned, that must stay alive until the call's work has finished.
 * use_average_share: bit 0 mean / sum, bits 4-5 objective (bit 1, share_noise False, is refused).
 * noise_*_steps, when given, are indexed by the DDIM STEP index: [n_steps, B, H*W, C-3] /
 * [n_steps, B*nb, H*W, 3]; else z comes from the counter-based generator (seed, sample_offset + b, t).
 * One captured HIP graph (U-Net + one element-wise update + the step counter) replayed per step when
 * use_graph; ws as cindm_ddpm2d_step. */
int  cindm_ddpm2d_sample_ddim(cindm_ddpm1d* sched, cindm_unet2d* u, float* x, int64_t B, int32_t nb,
                              int32_t use_average_share, int32_t n_steps, const int32_t* times,
                              const float* coefs, void* tab, size_t tab_bytes,
                              const float* noise_state_steps, const float* noise_boundary_steps,
                              uint64_t seed, int64_t sample_offset, void* ws, size_t ws_bytes,
                              void* stream, int32_t use_graph);
/* x_T for the 2-D path (sample_noise :775-785, :895): state channels shared over the boundaries of a design. */
int  cindm_fill_noise2d(float* x, int64_t B, int32_t nb, int32_t hw, int32_t channels,
                        int32_t padded_channels, uint64_t seed, int64_t sample_offset,
                        int32_t step_tag, void* stream);


/* ------------------------------------------------------------------ ForceUnet and the airfoil design gradient
 * Replaces ForceUnet.__init__/forward, model/diffusion_2d.py:411-486 (the surrogate of the lift / drag forces), and --
 * instead of torch.autograd.grad through it -- the design_fn of inference/inverse_design_2d.py:208-214 built from
 * force_fn :98-132 (sum_boundary = True) and overlap_fn :134-143.  Only input gradients exist (frozen weights).
 * Tensors: channel-last fp32; network input [images, H*W, channels]; sampler state [B*nb, H*W, CP] as cindm_ddpm2d_*. */
typedef struct cindm_forceunet cindm_forceunet;
typedef struct {
    int32_t dim;              /* 64                                         :414 */
    int32_t n_mults;          /* len(dim_mults) <= 4                        :417 */
    int32_t dim_mults[4];     /* (1, 2, 4, 8): the bottleneck must be 512 wide (final = Linear(512, 2), :458) */
    int32_t channels;         /* 4 = (pressure, boundary mask, 2 offsets)   :418 */
    int32_t image_size;       /* 64 = 8 * 2^(n_mults - 1): the coarsest level is 8 x 8 (other sizes: fewer levels) */
} cindm_forceunet_desc;

int  cindm_forceunet_create(const cindm_forceunet_desc* desc, cindm_forceunet** out);
void cindm_forceunet_destroy(cindm_forceunet* h);
int  cindm_forceunet_num_params(const cindm_forceunet* h);
int  cindm_forceunet_param_info(const cindm_forceunet* h, int idx, char* name, int name_cap, int64_t shape[4], int* ndim);
int  cindm_forceunet_set_param(cindm_forceunet* h, const char* key, const float* src, int64_t numel, int on_device);
/* Kernel-path options of a handle (as cindm_unet1d_set_option; pack options take effect at the next finalize): "h3" = 0 keeps the
 * forward 3x3 convolutions, "h3_bwd" = 0 the input-gradient ones, on the exact fp32 MFMA kernel instead of the
 * split-fp16 one (both paths meet the 2e-5 parity bound); "auto_range" = 0 skips the calibration forward of the range
 * rule; "range_fallback" (read-only) = 1 when that forward switched the handle to the fp32 convolutions; "stress" > 0:
 * pseudo-random delays before the producer -> consumer hand-overs of the persistent convolution kernel (race tests; run-time);
 * "la_fused" (0 = LinearAttention sites layer by layer), "gn_bwd_fused" (0 / 1 / 2: the GroupNorm + SiLU derivative), "ws_nosplit",
 * and the run-time options "no_exchange", "recover", "dbg", and "taps" (1 = the block outputs and their gradients of every
 * cindm_forceunet_forward / _grad / _vjp call stay readable for cindm_forceunet_tap: a residual chain's gradient is copied into each
 * tensor's own buffer instead of accumulating in one shared buffer -- out and dx bit for bit those of taps = 0, the same workspace
 * size; off on every sampling path). */
int  cindm_forceunet_set_option(cindm_forceunet* h, const char* key, int32_t value);
int  cindm_forceunet_get_option(const cindm_forceunet* h, const char* key, int32_t* value);
/* folds weight standardisation, packs forward and backward-data fragments, runs the range rule's calibration forward */
int  cindm_forceunet_finalize(cindm_forceunet* h, void* stream);
size_t cindm_forceunet_workspace_bytes(const cindm_forceunet* h, int64_t images, int32_t with_grad);
/* out[images, 2] = ForceUnet.forward(x)   (:460-486) */
int  cindm_forceunet_forward(cindm_forceunet* h, const float* x, float* out, int64_t images, void* ws, size_t ws_bytes, void* stream);
/* the same forward, and dx = d( sum_images lambda_force * |out[:,0]| + out[:,1] ) / dx  (what force_fn differentiates, :113-117) */
int  cindm_forceunet_grad(cindm_forceunet* h, const float* x, float lambda_force, float* out, float* dx, int64_t images,
                          void* ws, size_t ws_bytes, void* stream);
/* the same forward, and dx = d( sum_images dout[img] . out[img] ) / dx for a caller-given dout [images, 2]: the backward of
 * ForceUnet.forward under torch.autograd (cindm_amd.ForceUnet registers it), so force_fn of inverse_design_2d.py:98-132
 * runs against this model as written */
int  cindm_forceunet_vjp(cindm_forceunet* h, const float* x, const float* dout, float* out, float* dx, int64_t images,
                         void* ws, size_t ws_bytes, void* stream);
/* Test hook (option "taps" = 1): copy the block output `name` of the last forward / grad / vjp call (grad = 0), or the gradient of that
 * call's objective with respect to it (grad = 1; refused after a forward-only call), out of that call's workspace `ws` into dst as
 * [images, H*W, C]; shape receives (images, H*W, C), with dst == NULL only that.  Names as the reference's modules: init_conv,
 * downs.i.0 .. downs.i.3, mid_block1, mid_attn, mid_block2.  cindm_airfoil_design_grad and the chains lay out a workspace of
 * their own and serve no taps. */
int  cindm_forceunet_tap(cindm_forceunet* h, const char* name, int32_t grad, int64_t images, void* ws, float* dst,
                         int64_t dst_cap, int64_t shape[3], void* stream);
/* 1 when an in-kernel exchange between workgroups of this handle's kernels (the GroupNorm derivative on whole pixel rows, option
 * gn_bwd_fused = 2) timed out since the last call -- the affected gradients are NaN, never finite and wrong --, 0 otherwise; clears
 * the flag; synchronises `stream`.  cindm_ddpm2d_sample_force reads it at the end of the chain and re-runs ONCE from the kept x_T
 * on the exchange-free derivative (option recover = 0: returns an error instead); after cindm_forceunet_grad / _vjp /
 * cindm_airfoil_design_grad the caller polls it (the Python face does, and re-runs the call with option no_exchange = 1).
 * cindm_forceunet_recovered: how many chains / calls were re-run that way.  No reference counterpart. */
int  cindm_forceunet_status(cindm_forceunet* h, void* stream);
int  cindm_forceunet_recovered(const cindm_forceunet* h);
/* grad[B*nb, H*W, CP] = design_fn(x) = grad_force + lambda_overlap * grad_overlap (inverse_design_2d.py:208-214), the
 * tensor GaussianDiffusion.p_sample subtracts under "standard" / "standard-alpha" guidance (model/diffusion_2d.py:813-817).
 * frames = (real channels - 3) / 3; p_min / p_max: the pressure normalisation of the data set (:85-87). */
/* frames_per_pass: how many of the `frames` surrogate passes of one gradient run as one batch (a divisor of frames;
 * cindm_airfoil_design_grad uses the largest one whose workspace fits what it is given) */
size_t cindm_airfoil_design_workspace_bytes(const cindm_forceunet* h, int64_t B, int32_t nb, int32_t frames_per_pass);
/* sum_boundary: force_fn's switch (:98-132): 1 = the surrogate sees the clamped sum of a design's boundaries and the pressure
 * in simulator units (:100-120, the script's default); 0 = each copy's own boundary channels and the normalised pressure,
 * forces summed over the boundaries of a design (:122-130). */
int  cindm_airfoil_design_grad(cindm_forceunet* h, const float* x, int64_t B, int32_t nb, int32_t frames, int32_t CP,
                               float p_min, float p_max, float lambda_force, float lambda_overlap, int32_t downsampling_factor,
                               int32_t sum_boundary, float* grad, void* ws, size_t ws_bytes, void* stream);
/* Design-guided 2-D sampling with the airfoil objective inside the captured step (inference/inverse_design_2d.py:236-244
 * with design_guidance = "standard-alpha"; p_sample's guided tail model/diffusion_2d.py:806-845): per reverse step
 * g = cindm_airfoil_design_grad(x_t); x_{t-1} = p_sample(x_t) (as cindm_ddpm2d_sample); x_{t-1} -= eta[t] * g, with eta a
 * device table of `timesteps` floats (coeff_ratio * betas.flip(0)).  grad: a device buffer shaped like x; ws as
 * cindm_ddpm2d_sample, ws_force as cindm_airfoil_design_grad.  One hipGraph per call, replayed once per timestep.
 * SYNCHRONISES `stream` before it returns, with use_graph = 0 as well (since round 5): the chain's exchange flag is read at its end and a
 * timed-out chain is re-run once from the x_T kept in `ws` (round 6: a slice of the caller's workspace -- nothing is allocated); an eager
 * chain therefore cannot be enqueued asynchronously or captured by the caller.  The error word is cleared when it is read. */
int  cindm_ddpm2d_sample_force(cindm_ddpm1d* sched, cindm_unet2d* u, cindm_forceunet* f, float* x, int64_t B, int32_t nb,
                               int32_t use_average_share, const float* noise_state_steps,
                               const float* noise_boundary_steps, uint64_t seed, int64_t sample_offset,
                               int32_t t_start, int32_t t_end, int32_t frames, float p_min, float p_max,
                               float lambda_force, float lambda_overlap, int32_t down_factor, int32_t sum_boundary,
                               const float* eta, float* grad, void* ws, size_t ws_bytes, void* ws_force,
                               size_t ws_force_bytes, void* stream, int32_t use_graph);
/* Guided DDIM of the 2-D path with the airfoil objective inside the captured step (GaussianDiffusion.ddim_sample with
 * design_fn = ForceObjective, design_guidance = "standard-alpha"; the reference has no working 2-D DDIM, INTEGRATION.md defines it):
 * per DDIM step i, pair (t, t_next) = (times[i], times[i+1]),
 *   g = cindm_airfoil_design_grad(x_t);  x' = the update of cindm_ddpm2d_sample_ddim (same model_predictions, same draws);
 *   x_next = x' - weights[i] * g      (on the last pair, t_next = -1, too -- as p_sample shifts at t = 0)
 * with the update and the shift ONE element-wise launch.  weights [n_steps] is a HOST array like coefs (the caller sums
 * coeff_ratio * betas.flip(0) over the DDPM steps t_next+1 .. t that the DDIM step skips); it is copied into the 4th word of the
 * step's row of tab.  times / coefs / tab / noise_*_steps / use_average_share as cindm_ddpm2d_sample_ddim; frames .. sum_boundary,
 * grad (a device buffer shaped like x) and ws_force as cindm_ddpm2d_sample_force; ws as cindm_ddpm2d_step (its last slice keeps
 * x_T: nothing is allocated).  One hipGraph per call (surrogate gradient, U-Net, guided update, step counter), replayed n_steps
 * times.  SYNCHRONISES `stream` before it returns and re-runs a chain whose surrogate exchange timed out ONCE from x_T on the
 * exchange-free derivative, as cindm_ddpm2d_sample_force.  Every argument check precedes the first launch or copy. */
int  cindm_ddpm2d_sample_ddim_force(cindm_ddpm1d* sched, cindm_unet2d* u, cindm_forceunet* f, float* x, int64_t B, int32_t nb,
                                    int32_t use_average_share, int32_t n_steps, const int32_t* times, const float* coefs,
                                    const float* weights, void* tab, size_t tab_bytes, const float* noise_state_steps,
                                    const float* noise_boundary_steps, uint64_t seed, int64_t sample_offset,
                                    int32_t frames, float p_min, float p_max, float lambda_force, float lambda_overlap,
                                    int32_t down_factor, int32_t sum_boundary, float* grad, void* ws, size_t ws_bytes,
                                    void* ws_force, size_t ws_force_bytes, void* stream, int32_t use_graph);

/* ------------------------------------------------------------------ n-body re-simulation of designs
 * Stands where the reference calls utils.simulation (utils.py:1071-1125, a pymunk / pygame program): B independent scenes of n_bodies
 * equal, frictionless, perfectly elastic discs of radius `radius` in a box whose walls are segments of half-thickness wall_radius on
 * x = 0, width, y = 0, height (add_body / add_walls, utils.py:1009-1033), no gravity, no damping, advanced by the continuous-time
 * dynamics: centres live in [lo, hi] = [radius + wall_radius, extent - radius - wall_radius] per axis; inside a frame of length dt the
 * earliest wall or pair contact is found in closed form, every body is moved to it, the contact is resolved (wall: that velocity
 * component changes sign; pair: the normal components exchange) and the search repeats, at most max_events_per_frame times per frame,
 * after which the rest of the frame is ballistic.  NOT an emulation of Chipmunk's fixed-step impulse solver: trajectories differ from
 * pymunk's by about one step's travel per contact (DESIGN 4.10b states the rule in full and what has not been measured).
 * features [B, n_bodies, 4] = (x, y, vx, vy) and out [B, n_steps, n_bodies, 4] are DEVICE float64 (the reference's simulator returns
 * float64); frame i of out is the state at time i * dt, frame 0 the input.  status [B], DEVICE: bit 1 = the input starts with an
 * overlap or a centre outside [lo, hi]; 2 = the event cap was reached in some frame; 4 = coincident centres at a pair event (skipped,
 * that frame ends ballistically); 8 = a non-finite input (every output row of that design is NaN, nothing else is set).  events [B],
 * DEVICE: contacts resolved over the n_steps - 1 frames stepped.  Asynchronous on `stream`; no allocation, no handle, no workspace.
 * Checked before the launch: non-null pointers, 1 <= n_bodies <= 8, 1 <= n_steps <= 65535, 1 <= B <= 2^22, radius > 0,
 * wall_radius >= 0, hi > lo on both axes, dt > 0 and finite, 1 <= max_events_per_frame <= 4096. */
typedef struct {
    double width, height, radius, wall_radius, dt;
    int32_t max_events_per_frame;
} cindm_nbody_desc;
int  cindm_nbody_simulate(const cindm_nbody_desc* desc, const double* features, int64_t B, int32_t n_bodies, int32_t n_steps,
                          double* out, int32_t* status, int32_t* events, void* stream);

/* ------------------------------------------------------------------ multi-GPU: the one collective of the path
 * the design batch is sharded over the ranks with no communication inside the reverse loop;
 * the final designs are all-gathered ONCE.  The reference has no counterpart (inference/inverse_design_diffusion_1d.py:161 is
 * single-device).  These entry points call RCCL (librccl.so, resolved with dlopen at first use: the library itself has no link
 * dependency on it) over xGMI:
 *   cindm_comm_unique_id   ncclGetUniqueId: 128 opaque bytes made by rank 0 and handed to every rank by the caller's own
 *                          rendezvous (the Python face broadcasts them over the torch.distributed group it already has);
 *   cindm_comm_init        ncclCommInitRank on the CURRENT device -> an opaque communicator;
 *   cindm_all_gather_designs   ncclAllGather(float): every rank contributes per_rank_elems floats at `local`, `out` receives
 *                          world * per_rank_elems floats in rank order; asynchronous on `stream`;
 *   cindm_comm_destroy     ncclCommDestroy.
 * Ragged shards are padded to the largest one by the caller (cindm_amd/dist.py). */
typedef struct cindm_comm cindm_comm;
int  cindm_comm_unique_id(unsigned char id[128]);
int  cindm_comm_init(const unsigned char id[128], int32_t world, int32_t rank, cindm_comm** out);
int  cindm_comm_world(const cindm_comm* c);
int  cindm_all_gather_designs(const float* local, float* out, int64_t per_rank_elems, cindm_comm* comm, void* stream);
void cindm_comm_destroy(cindm_comm* c);

#ifdef __cplusplus
}
#endif
#endif /* CINDM_HIP_H */
