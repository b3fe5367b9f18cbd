/*
 * stereonet_hip.h — C ABI of libstereonet_hip.so, the MI355X (gfx950) replacement
 * for the Horizon BPU execution behind hobot_stereonet's StereonetNode.
 *
 * What this boundary replaces in the reference (paths under /root/reference):
 *   - hobot::dnn_node::DnnNode::Init()  -> model load     stereonet_infer/src/stereonet_node.cpp:44
 *   - DnnNode::GetModelInputSize / Model::Get*TensorProperties
 *                                                          stereonet_node.cpp:45,57-103
 *   - DnnNode::Run(inputs, output, is_sync, -1, -1)        stereonet_node.cpp:812 (async),
 *                                                          :177,:584,:968 (sync)
 *   - PreProcess::CvtNV12Data2Tensors (optional fused)     stereonet_infer/src/preprocess.cpp:913-1059
 *   - the NV12 side-by-side split in FeedImg (optional)    stereonet_node.cpp:705-738
 * The reference reaches all of these through the closed `dnn_node`/`libdnn`
 * (hbDNN*, hbSys*) API; hobot_stereonet_amd/csrc/compat/ re-implements exactly
 * the members the reference touches on top of the functions below (see
 * INTEGRATION.md for the binding a maintainer adds).
 *
 * Conventions: plain C types only; every function returns int, 0 = ok, <0 =
 * error (the reference's -1 convention, stereonet_infer/include/parser.h:37-39);
 * no exceptions cross the boundary.  Buffers are caller-owned.  `mem` says
 * whether data pointers are host (SN_MEM_HOST) or HIP device (SN_MEM_DEVICE)
 * memory.  `stream` is a hipStream_t passed as void* (NULL = the handle's own
 * stream, and the call returns after completion; non-NULL with SN_MEM_DEVICE =
 * work is only enqueued on that stream).  A handle is bound to one GPU; calls on
 * one handle must not overlap in time except sn_submit/sn_wait, which are
 * thread-safe (task_num requests in flight, stereonet_node.cpp:144).
 *
 * Tensor contract (unchanged from the reference):
 *   input  int8  NCHW [n][6][H][W]: L-Y, L-"U", L-"V", R-Y, R-"U", R-"V"; value = byte ^ 0x80
 *          (preprocess.cpp:999-1003,1033-1040)
 *   output int32 NCHW [n][1][H][W]: raw; disparity_px = raw * out_scale * 16 * 12 — the reference's literal
 *          factor (stereonet_node.cpp:282-288, parser.cpp:84-86, publisher_member_function.py:73-75) for every
 *          dmax, so the unmodified consumers recover pixels whatever D the model was built for
 *   optional float output [n][H][W]: disparity in px before int32 quantisation.
 */
#ifndef STEREONET_HIP_H_
#define STEREONET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sn_handle sn_handle;

/* Version of this binary interface.  4 = SN_ERR_RANGE exists and sn_refine_stats ends in nonfinite_px / nonfinite_low_px;
 * 3 = SN_PREC_AUTO exists and is what 0 ("default") selects, sn_io_info ends in
 * precision_selected, sn_get_refine_stats / sn_auto_* exist; 2 = the SN_PREC_* numbering below with 0 = SN_PREC_F16 and
 * exact fp32 = 3; version 1 (round 1) had 0 = exact fp32.  A caller built against an older header compares
 * SN_ABI_VERSION with sn_abi_version() at start-up instead of silently running in another arithmetic. */
#define SN_ABI_VERSION 4
int sn_abi_version(void);

enum {
  SN_OK = 0,
  SN_ERR_ARG = -1,       /* null / out-of-range argument, geometry mismatch          */
  SN_ERR_FILE = -2,      /* model_file missing or unreadable (stereonet_node.cpp:131) */
  SN_ERR_FORMAT = -3,    /* not an SNW1 weight file / wrong architecture header       */
  SN_ERR_DEVICE = -4,    /* HIP runtime error or no gfx950 device                     */
  SN_ERR_NOMEM = -5,
  SN_ERR_BUSY = -6,      /* sn_submit: no free task slot within the timeout           */
  SN_ERR_TICKET = -7,    /* sn_wait: unknown or already-consumed ticket               */
  SN_ERR_RANGE = -8      /* the maps were written, but the arithmetic that computed them left the range of fp16: see below */
};
/* SN_ERR_RANGE.  SN_PREC_F16 and SN_PREC_F16X3 (and so SN_PREC_AUTO) store the 32-channel activations between layers as fp16,
 * or as a hi/lo pair of fp16 — the low-resolution branch in both modes alike.  fp16 ends at 65504: a model whose activations
 * pass that (a trained, BN-folded checkpoint is under no obligation not to) leaves inf / NaN in those tensors, and the relu of
 * the heads would hand back a finite map of zeros — "infinitely far" on the wire.  Every head kernel therefore counts the
 * pixels whose disparity is not finite before its relu, every soft-argmin kernel the pixels with a non-finite cost
 * (sn_refine_stats: nonfinite_px, nonfinite_low_px; nothing feeds back into the maps).  A non-zero count makes the call's
 * residual_px +inf, which takes an SN_PREC_AUTO handle to SN_PREC_F16X3 (a blocking call is repeated there), and a blocking
 * call — sn_wait included — whose returned maps come from an arithmetic with a non-zero count returns SN_ERR_RANGE instead of
 * SN_OK: the outputs are written, and they are not to be used.  A call that only enqueues work shows the counts in
 * sn_get_refine_stats once its statistic is folded in.  Use SN_PREC_FP32 for such a model. */

enum { SN_MEM_HOST = 0, SN_MEM_DEVICE = 1 };

/* Arithmetic of the convolution contractions.  All variants accumulate in fp32. */
enum {
  SN_PREC_DEFAULT = 0,   /* a zero-initialised or NULL sn_config selects SN_PREC_AUTO             */
  SN_PREC_F16X3 = 1,     /* refinement tower on fp16 MFMA with hi/lo operand split (3 MFMAs per   */
                         /* product, ~2^-22 relative): fp32-class accuracy at 3/16 of the fp32    */
                         /* MFMA cost; activations stored as two fp16 tensors                     */
  SN_PREC_F16 = 2,       /* refinement tower on plain fp16 MFMA operands (3x3 weights rounded per  */
                         /* kernel so that every kernel's tap sum survives: no coherent offset);  */
                         /* low-resolution branch on 22-bit split fp16 operands.  Its error is     */
                         /* proportional to what the refinement adds to the map: over 8 weight    */
                         /* draws (profiles/r05_epe_sensitivity_*.txt) EPE vs the fp32 oracle is    */
                         /* 1.8e-4 .. 8.3e-4 px per pixel of mean |D r|, i.e. < 1e-3 px is only    */
                         /* GUARANTEED up to ~1.1 px of mean residual at 1280x720 (typically up   */
                         /* to ~2 px); a hierarchical model holds at head gain 1 only.  Forcing    */
                         /* this mode is the caller's statement that the model is inside that.    */
  SN_PREC_FP32 = 3,      /* exact fp32 MFMA (v_mfma_f32_32x32x2_f32) everywhere                   */
  SN_PREC_AUTO = 4       /* the default: SN_PREC_F16 while the model stays inside the fp16 tower's */
                         /* envelope, SN_PREC_F16X3 otherwise.  Every head kernel sums |D r| (the  */
                         /* refinement statistic, sn_get_refine_stats); the first call of a handle */
                         /* also runs one pair in both arithmetics and measures their distance.    */
                         /* A call whose statistic (or self-check) predicts EPE > 1e-3 px is       */
                         /* REPEATED in SN_PREC_F16X3 before it returns, and the handle stays      */
                         /* there until the statistic has been back inside 0.8 of the envelope    */
                         /* for 8 calls.  Calls that only enqueue work (device buffers + a caller */
                         /* stream) cannot be repeated: the first such call of a handle blocks    */
                         /* for the self-check, later ones act on the statistic of the call        */
                         /* before (sn_auto_* below is the state machine, pure functions).  The    */
                         /* rule and the bound are PER CALL: a batch is judged on the mean         */
                         /* residual of its pairs and keeps the MEAN EPE of its pairs below 1e-3   */
                         /* px; one hard pair among calm ones can stay in fp16 above it (measured  */
                         /* worst pair: 1.03e-3 px in a call of 8 at a mean of 4.6e-4 px,          */
                         /* profiles/auto_sequences.txt).  A per-pair statistic is future work.    */
};

typedef struct sn_config {
  int device;        /* HIP device ordinal, -1 = current device                                 */
  int max_batch;     /* largest n for sn_infer_batch; <=0 -> 1                                   */
  int width;         /* 0 = take from the model file header                                      */
  int height;        /* 0 = take from the model file header                                      */
  int dmax;          /* max disparity D (multiple of 16, <= 256); 0 = from the model file        */
  int precision;     /* SN_PREC_*; 0 = SN_PREC_AUTO                                               */
  int task_num;      /* async slots for sn_submit; <=0 -> 4 (stereonet_node.cpp:144)              */
  int refine_chunk;  /* pairs per refinement-tower launch; <=0 -> sized by work per launch, about    */
                     /* 5.5 Mpx (6 at 1280x720, 8 at 1248x384, max 8); the per-layer forms           */
                     /* (SN_FUSE=0, SN_PREC_F16X3, SN_PREC_FP32) keep the Infinity-Cache sizing       */
  int piece;         /* pairs per low-resolution piece of the pipeline; <=0 -> 16 (SN_PREC_FP32: the    */
                     /* first piece of a call is 2-4 pairs, nothing overlaps its low-res branch)     */
} sn_config;

typedef struct sn_io_info {
  int width, height, dmax;
  int in_channels;        /* 6 */
  int max_batch, precision, task_num, device;
  float out_scale;        /* 2.60443857769133e-6 (stereonet_node.cpp:282) */
  size_t in_bytes;        /* per pair: 6*H*W  (int8)  */
  size_t out_bytes;       /* per pair: 4*H*W  (int32) */
  double flops_per_pair;  /* algorithmic conv FLOPs (2*MAC), DESIGN.md §5 */
  int refine_chunk;       /* pairs per refinement-tower launch actually in use */
  int piece;              /* pairs per low-resolution piece actually in use    */
  int tower_streams;      /* tower chunks in flight (1 or 2)                   */
  int refine_levels;      /* 1 = single-scale refinement; 4 = hierarchical (towers at 1/8, 1/4, 1/2, 1), as the
                           * model file says (weights.py: header word 72) */
  int precision_selected; /* arithmetic the NEXT call runs in: = precision unless that is SN_PREC_AUTO
                           * (then SN_PREC_F16 or SN_PREC_F16X3) */
} sn_io_info;

/* DnnNode::Init + Model introspection ------------------------------------------------------- */
int sn_create(const char *model_file, const sn_config *cfg, sn_handle **out);
int sn_destroy(sn_handle *h);
int sn_get_io_info(const sn_handle *h, sn_io_info *info);
const char *sn_strerror(int code);
const char *sn_last_error(const sn_handle *h);   /* detail of the last failure on this handle; h = NULL: of the
                                                  * last failed sn_create on the calling thread.  Safe beside calls on
                                                  * other threads: the text is copied for the calling thread and stays
                                                  * valid until its next sn_last_error */

/* Refinement statistic and SN_PREC_AUTO --------------------------------------------------------------------------
 * The reference loads an opaque model_file and only checks that it exists (stereonet_node.cpp:131-136); whether the
 * fp16 tower keeps north_star's 1e-3 px on it depends on how far its refinement moves the map.  Every head kernel
 * therefore accumulates the sum of |D_k r_k| over the pixels it writes (level k of the refinement, in level-k pixels;
 * one 64-bit fixed-point atomic per wave, outputs bit-unchanged), all precision modes. */
typedef struct sn_refine_stats {
  int levels;                       /* refinement levels of the model (1 or 4)                                        */
  int precision;                    /* as configured (SN_PREC_*)                                                      */
  int precision_selected;           /* arithmetic the next call runs in (differs from `precision` under SN_PREC_AUTO)  */
  int precision_last;               /* arithmetic the most recent call's maps were computed in                        */
  uint64_t calls, pairs;            /* completed calls / stereo pairs since sn_create (every entry point)             */
  uint64_t switches;                /* SN_PREC_AUTO: changes of arithmetic                                            */
  uint64_t reruns;                  /* SN_PREC_AUTO: calls repeated in SN_PREC_F16X3 before they returned              */
  double level_px[4];               /* last call: mean |D_k r_k| of level k (0 = full resolution), level-k pixels      */
  double residual_px;               /* last call: sum_k 2^k level_px[k] = full-resolution pixels the refinement adds;  */
                                    /* +inf when a count below is non-zero                                            */
  double running_px;                /* exponential mean of residual_px over the calls (weight 1/4)                    */
  double envelope_px;               /* SN_PREC_F16 is trusted while residual_px stays below this (shape class)         */
  double limit_px;                  /* the threshold in force (sn_auto_limit_px)                                      */
  double selfcheck_epe_px;          /* mean |F16 - F16X3| of the self-check pair, < 0 = not measured                   */
  double selfcheck_residual_px;     /* residual_px of that pair                                                       */
  uint64_t nonfinite_px[4];         /* last call: pixels of level k whose disparity was not finite before the head's relu */
                                    /* (+ partial sums of |D_k r_k| that were not): SN_ERR_RANGE                          */
  uint64_t nonfinite_low_px;        /* last call: low-resolution pixels with a non-finite matching cost                  */
} sn_refine_stats;
int sn_get_refine_stats(sn_handle *h, sn_refine_stats *out);

/* SN_PREC_AUTO's decision as pure functions (no GPU; tests/test_auto_precision.py).  sn_auto_observe folds the statistic of
 * one finished call in and returns the arithmetic of the next one; a caller that ran the call in SN_PREC_F16 and gets
 * SN_PREC_F16X3 back repeats the call.
 *   limit: envelope_px (the shape class's envelope = the budget over the WORST error-per-pixel of the measured weight
 *          draws) until the self-check has measured THIS model's error per pixel of residual (epe_per_px); then
 *          min(envelope_px, SN_AUTO_BUDGET_PX / epe_per_px).  The self-check only TIGHTENS the limit: it measures one pair,
 *          the first the handle sees in SN_PREC_F16, and the error per pixel of residual depends on the frame (a handle
 *          calibrated on a calm frame used to trust a later frame with 3 times its residual, and returned an fp16 map at
 *          1.03e-3 px for it: tests/test_gpu_auto_sequences.py, profiles/auto_sequences.txt).
 *   F16 -> F16X3: residual > limit (at once).  F16X3 -> F16: SN_AUTO_CALM_CALLS consecutive calls with residual <
 *   SN_AUTO_REENTRY * limit. */
#define SN_AUTO_BUDGET_PX 0.85e-3   /* of north_star's 1e-3 px: the rest is SN_PREC_F16X3's own distance to the oracle */
#define SN_AUTO_REENTRY 0.8
#define SN_AUTO_CALM_CALLS 8
typedef struct sn_auto_state {
  int mode;             /* SN_PREC_F16 or SN_PREC_F16X3: arithmetic of the next call                              */
  int calm;             /* consecutive SN_PREC_F16X3 calls whose residual sat inside the re-entry band            */
  double envelope_px;   /* measured envelope of the shape class (sn_auto_envelope_px)                             */
  double epe_per_px;    /* self-check: mean |F16 - F16X3| per pixel of residual; 0 = not measured                 */
  double running_px;    /* exponential mean of the residual, < 0 before the first call                            */
  uint64_t switches;
} sn_auto_state;
double sn_auto_envelope_px(int refine_levels);          /* 1: single-scale; 4: hierarchical                        */
int sn_auto_init(sn_auto_state *s, int refine_levels);
double sn_auto_limit_px(const sn_auto_state *s);
int sn_auto_observe(sn_auto_state *s, double residual_px);   /* returns the new s->mode                            */

/* DnnNode::Run, synchronous form (stereonet_node.cpp:968) ----------------------------------- */
/* out_i32 and out_disp may each be NULL (but not both). */
int sn_infer_i8(sn_handle *h, const int8_t *in_nchw6, int32_t *out_i32, float *out_disp,
                int mem, void *stream);
int sn_infer_batch(sn_handle *h, int n, const int8_t *in_nchw6, int32_t *out_i32, float *out_disp,
                   int mem, void *stream);

/* PreProcess::CvtNV12Data2Tensors on the GPU (preprocess.cpp:913-1059), bit-exact, including the
 * reference's planar-I420 reading of the NV12 chroma (preprocess.h:131-133). */
int sn_preprocess_nv12(sn_handle *h, const uint8_t *left_nv12, const uint8_t *right_nv12,
                       int w, int h_px, int8_t *out_nchw6, int mem, void *stream);
/* FeedImg's split (stereonet_node.cpp:705-738) + CvtNV12Data2Tensors + Run in one call: takes the
 * raw 2W x H side-by-side NV12 message payload.  out_tensor (nullable) receives the int8 model
 * input the reference would have built. */
int sn_infer_sbs_nv12(sn_handle *h, const uint8_t *sbs_nv12, int w2, int h_px, int32_t *out_i32,
                      float *out_disp, int8_t *out_tensor, int mem, void *stream);

/* The same split + mapping for n side-by-side frames (n * 3*H*W bytes -> n * 6*H*W bytes), no inference: the batched
 * ingest of a streaming host (bench.py --stream) that ships camera frames instead of model tensors. */
int sn_preprocess_sbs_nv12_batch(sn_handle *h, int n, const uint8_t *sbs_nv12, int w2, int h_px, int8_t *out_nchw6,
                                 int mem, void *stream);

/* DnnNode::Run, asynchronous form (stereonet_node.cpp:812): host buffers only.  sn_submit copies
 * the input and returns at once with a ticket; up to task_num tickets are in flight;
 * timeout_ms < 0 waits for a free slot forever (the reference passes -1).  sn_wait blocks until the
 * ticket's pair is done, fills the host outputs given at submit, and reports the device time.  Once sn_wait has found
 * the ticket, every return consumes it and frees its slot; a return with a device error (not SN_ERR_RANGE, which hands the
 * maps over) leaves the host outputs unwritten. */
int sn_submit(sn_handle *h, const int8_t *in_nchw6_host, int32_t *out_i32_host, float *out_disp_host,
              int timeout_ms, uint64_t *ticket);
/* The same with FeedImg's raw 2W x H side-by-side NV12 frame as the input (stereonet_node.cpp:705-738 + preprocess.cpp:
 * 913-1059 run on the GPU): half the host-to-device bytes of sn_submit. */
int sn_submit_nv12(sn_handle *h, const uint8_t *sbs_nv12_host, int w2, int h_px, int32_t *out_i32_host,
                   float *out_disp_host, int timeout_ms, uint64_t *ticket);
int sn_wait(sn_handle *h, uint64_t ticket, float *infer_ms);
int sn_synchronize(sn_handle *h);

/* Multi-GPU form: the independent pairs of one batch sharded over the GPUs of one node -------------------------
 * The reference keeps task_num = 4 independent frames in flight behind one Run() call site
 * (stereonet_node.cpp:144,812); this spreads such units of work over devices instead: contiguous shards (the first
 * n % ndev shards get one extra pair), one host thread + one engine per GPU, weights replicated, NO data-path
 * collective; the single exchange is the gather of the maps to the root.  cfg->device is ignored, cfg->max_batch is
 * the largest TOTAL n; devices == NULL selects 0..ndev-1.
 *   sn_mgpu_infer_batch         host buffers: every device copies its shard in and its maps out — the host is the root.
 *   sn_mgpu_infer_batch_device  in_per_device[k] = shard k resident on device k; maps gathered in batch order into
 *                               out_* on device 0 over xGMI: one grouped RCCL ncclSend/ncclRecv exchange per batch
 *                               (the default when ndev > 1 and librccl loads), or hipMemcpyPeerAsync from each peer over
 *                               its own link (fallback; SN_MGPU_GATHER=peer forces it).  = submit + wait below.
 *   sn_mgpu_submit_device /     the asynchronous form of the same (the reference's async Run with task slots): returns a
 *   sn_mgpu_wait                ticket once every device has its shard enqueued; SN_MGPU_SLOTS = 2 tickets may be in
 *                               flight (per-device staging is double buffered), so the gather of batch k overlaps the
 *                               compute of batch k + 1.  Inputs and root buffers belong to the call until the wait.
 * Results are bit-identical to sn_infer_batch on one GPU (same kernels, no cross-pair reduction). */
typedef struct sn_mgpu sn_mgpu;
int sn_mgpu_shard(int n, int ndev, int k, int *first, int *count);         /* pure shard arithmetic */
int sn_mgpu_create(const char *model_file, const sn_config *cfg, const int *devices, int ndev, sn_mgpu **out);
int sn_mgpu_destroy(sn_mgpu *m);
int sn_mgpu_get_info(const sn_mgpu *m, int *ndev, int *per_device_batch, int *gather_kind /* 1 peer copy, 2 RCCL */);
int sn_mgpu_get_handle(sn_mgpu *m, int k, sn_handle **h);                  /* the engine of shard k (borrowed) */
/* The borrowed engine shares its workspace with the sn_mgpu_* calls: use it (sn_infer_*, sn_submit, ...) only while
 * no sn_mgpu_submit_device ticket is in flight and no other sn_mgpu_* call runs; sn_mgpu_infer_batch itself returns
 * SN_ERR_BUSY while tickets are outstanding. */
int sn_mgpu_infer_batch(sn_mgpu *m, int n, const int8_t *in_nchw6_host, int32_t *out_i32_host, float *out_disp_host);
int sn_mgpu_infer_batch_device(sn_mgpu *m, int n, const int8_t *const *in_per_device, int32_t *out_i32_root,
                               float *out_disp_root);
int sn_mgpu_submit_device(sn_mgpu *m, int n, const int8_t *const *in_per_device, int32_t *out_i32_root,
                          float *out_disp_root, uint64_t *ticket);      /* SN_ERR_BUSY: two tickets in flight */
int sn_mgpu_wait(sn_mgpu *m, uint64_t ticket);                            /* SN_ERR_TICKET: unknown / consumed   */
const char *sn_mgpu_last_error(const sn_mgpu *m);
/* The ticket / buffer-slot bookkeeping of the asynchronous form as pure functions (no GPU; tests): tickets count from
 * 1, ticket t uses slot t % SN_MGPU_SLOTS, a slot is busy from submit to the wait of its ticket. */
#define SN_MGPU_SLOTS 2
typedef struct sn_mgpu_ring {
  uint64_t next;
  uint64_t slot_ticket[SN_MGPU_SLOTS];
} sn_mgpu_ring;
int sn_mgpu_ring_init(sn_mgpu_ring *r);
int sn_mgpu_ring_submit(sn_mgpu_ring *r, uint64_t *ticket, int *slot);
int sn_mgpu_ring_wait(sn_mgpu_ring *r, uint64_t ticket, int *slot);

/* Measurement hooks (bench.py): per-stage device time of the most recent sn_infer_batch, taken
 * with hipEvents on the stream the kernels ran on.  Stage ids: */
enum {
  SN_STAGE_FEATURES = 0,   /* Siamese tower, both eyes            */
  SN_STAGE_AGGREGATE = 1,  /* cost volume + 3-D convs + soft-argmin */
  SN_STAGE_REFINE = 2,     /* upsample + refinement tower + output epilogue */
  SN_STAGE_REFINE_CONV = 3,/* the span of the 12 C->C 3x3 convs inside REFINE (first chunk) */
  SN_STAGE_TOTAL = 4,
  SN_STAGE_DOMINANT = 5,   /* the launches sn_get_dominant_kernel describes, first refinement chunk, timed one by one
                            * (the streamed residual blocks); equals REFINE_CONV when the tower runs layer by layer */
  SN_STAGE_COUNT = 6
};
int sn_set_profiling(sn_handle *h, int enable);
int sn_get_stage_ms(sn_handle *h, float *ms, int count);
/* launches of the dominant kernel in the last call and its algorithmic FLOPs / HBM bytes per launch */
int sn_get_dominant_kernel(sn_handle *h, char *name, size_t name_cap, int *launches,
                           double *flops_per_launch, double *bytes_per_launch);

/* Parity hooks (tests only; they run the product kernels on caller data, host memory) -------- */
/* The grid of the parity hooks.  Every hot kernel is persistent: its launcher sizes the grid from the CU count, and a
 * workgroup walks several tiles (or a share of the streamed blocks' flat rows).  sn_dbg_set_grid_cus makes the sn_dbg_* hooks
 * (and nothing else: the forward pass never reads it) hand their launchers `cus` in place of the device's CU count, so that a
 * small tensor runs the tile loops, queue and share boundaries a full-size one does.  cus = 1 .. the device's CU count, 0
 * restores the default; SN_ERR_ARG otherwise.  A hook whose launcher builds its grid in XCD bands of 8 (the split-slot
 * convolutions, sn_dbg_conv3d's slot forms, sn_dbg_agg_tail, sn_dbg_down01_n, sn_dbg_ref_conv_f16_n / _f16x3_n and the two-launch
 * forms of the blocks) returns SN_ERR_ARG with a message while the value is no multiple of 8.
 * sn_dbg_last_launch: workgroups and work units (tiles; half tiles for k_ref_conv_f32; flat rows for the streamed blocks) of
 * the last launch of the last hook call that went through a persistent launcher (0, 0 for one that did not). */
int sn_dbg_set_grid_cus(sn_handle *h, int cus);
int sn_dbg_last_launch(sn_handle *h, int *wgs, int *units);
/* The kernel a convolution hook runs (`form` of sn_dbg_conv2d_n and sn_dbg_conv3d; any other value: SN_ERR_ARG):
 * F32 = the generic fp32-operand MFMA kernel.  TOWER32 (conv2d; cin 32, 3x3, w % 4 == 0) = the fp32 tower kernel
 * k_ref_conv_f32; other shapes run as F32.  SLOTS (cin 32, dilation 1) = the split-operand kernel of the fp16 modes on
 * split-slot tensors (hi / lo fp16, their low-resolution activation format; the hook converts to and from that layout)
 * through the weights-stationary k_conv_x3s.  SLOTS_DMA = the same operands in zero-bordered tensors: k_feat_x3s_dma (3x3;
 * a residual is added in place, as the feature tower does), k_down_x3s_dma (5x5 stride 2, no residual) or k_agg_x3s_dma
 * (conv3d); the hook also checks that the borders stay zero. */
enum { SN_DBG_CONV_F32 = 0, SN_DBG_CONV_TOWER32 = 1, SN_DBG_CONV_SLOTS = 2, SN_DBG_CONV_SLOTS_DMA = 3 };
/* The hooks with a leading n run n images (pairs for the down-convs) in ONE launch, as the pipeline batches them.
 * lrelu: 0, or 1 = LeakyReLU.  residual (nullable): added in place, as the pipeline does.
 * sn_dbg_conv2d_n: one C->32 convolution, 3x3 stride 1 or 5x5 stride 2: in [n][cin][h][w] fp32, wt [32][cin][k][k],
 * residual / out [n][32][ho][wo]. */
int sn_dbg_conv2d_n(sn_handle *h, int n, const float *in, int cin, int h_px, int w, const float *wt,
                    const float *bias, int k, int stride, int dil, int lrelu, int form, const float *residual,
                    float *out);
/* one 3x3x3 32->32 conv3d (+bias): in [32][d][h][w] -> out [32][d][h][w]; form F32, SLOTS or SLOTS_DMA */
int sn_dbg_conv3d(sn_handle *h, const float *in, int d, int h_px, int w, const float *wt,
                  const float *bias, int lrelu, int form, float *out);
/* the first down-conv (3->32, 5x5, stride 2, no activation) of both eyes through the fp16-MFMA kernel of the fp16
 * modes: in6 int8 [n][6][h][w] (model input), wt [32][3][5][5], out [2n][32][ho][wo] with ho/wo = ceil16(h|w)/2; tc = 32 */
int sn_dbg_down0_n(sn_handle *h, int n, const int8_t *in6, int h_px, int w, const float *wt, const float *bias, int tc,
                   float *out);
/* The rounding SN_PREC_F16 applies to the 3x3 weights of its refinement towers at model load (host only, no device):
 * w [nkernels][9] fp32 -> out [nkernels][9], every value one of the two fp16 numbers enclosing its input, chosen per kernel
 * so that the SUM of the nine rounding errors is smallest (csrc/stereonet_hip.hip round_kernel_sum_preserving;
 * SN_W_ROUND=rne restores round-to-nearest in the engine). */
int sn_dbg_round_kernels_f16(const float *w, int nkernels, float *out);
/* The first TWO down-convs (3->32 and 32->32, both 5x5 stride 2, no activation between them) folded into one 13x13
 * stride-4 convolution, as the fp16 modes run them (csrc/sn_down01.hpp; SN_DOWN01=0 restores the two kernels).
 * sn_dbg_compose_down01 is the host-side fold alone (no device): w0 [32][3][5][5], b0 [32], w1 [32][32][5][5], b1 [32]
 * -> weff [9][32][3][13][13], beff [9][32]; class = 3 * row class + column class, each {first, inner, last} row / column
 * of the quarter-resolution map (down-conv 1's zero padding of the half-resolution map drops taps there).
 * sn_dbg_down01_n runs both eyes through the pipeline's two kernels: in6 int8 [n][6][h][w] -> out [2n][32][ho][wo] with
 * ho/wo = ceil16(h|w)/4. */
int sn_dbg_compose_down01(const float *w0, const float *b0, const float *w1, const float *b1, float *weff,
                          float *beff);
int sn_dbg_down01_n(sn_handle *h, int n, const int8_t *in6, int h_px, int w, const float *w0, const float *b0,
                    const float *w1, const float *b1, float *out);
/* The tower hooks (sn_dbg_refin_n, sn_dbg_ref_conv_*, sn_dbg_ref_block_*, sn_dbg_ref_tail_f16) take fp32 host tensors
 * [n][32][h][w], convert them to the kernels' fp16 NCHW8c layout and back (SN_PREC_F16X3: hi / lo), and allocate them as the
 * pipeline does ([front rows | tensor | slack]).  A tensor that is not an input (everything except the input and the in-place
 * residual) starts with the 0xff pattern (fp16 NaN) in its valid area, and after the launch the zero border of all n images,
 * the front rows and the slack of EVERY tensor are read back: SN_ERR_DEVICE with a message if any of them changed.  dil = 1, 2,
 * 4 or 8; a tensor too large for 32-bit byte offsets: SN_ERR_ARG.
 * sn_dbg_refin_n: the refinement input conv (4->32, 3x3, LeakyReLU): disp_low fp32 [n][hp/16][wp/16] (full-resolution px / 16
 * units as the soft-argmin head writes it), in6 int8 [n][6][h][w], wt [32][4][3][3]; out [n][32][hp][wp] (hp/wp = ceil16);
 * split != 0 selects the hi/lo output of SN_PREC_F16X3. */
int sn_dbg_refin_n(sn_handle *h, int n, const float *disp_low, const int8_t *in6, int h_px, int w, int dmax,
                   const float *wt, const float *bias, int split, float *out);
/* one 32->32 3x3 conv through the fp16 refinement-tower kernel (needs an engine created in an fp16 mode); tile_w = 64 / 32
 * forces the 8x64 / 8x32 tile variant of the dilation-1 / -2 kernel, 0 = the width the engine picks for the launch from its
 * tile count; and the same layer through the split-operand (SN_PREC_F16X3) kernel */
int sn_dbg_ref_conv_f16_n(sn_handle *h, int n, const float *in, int h_px, int w, const float *wt, const float *bias,
                          int dil, int lrelu, int tile_w, const float *residual, float *out);
int sn_dbg_ref_conv_f16x3_n(sn_handle *h, int n, const float *in, int h_px, int w, const float *wt, const float *bias,
                            int dil, int lrelu, const float *residual, float *out);
/* one residual block y = lrelu(x + conv2(lrelu(conv1(x)+b1)) + b2) of the fp16 tower (needs an engine created in an fp16
 * mode), and the same block on split operands (SN_PREC_F16X3).  form 0 = two convolution launches, 1 = the row-streaming fused
 * kernel the pipeline runs by default (sn_stream_block.hpp, sn_stream_block_x3.hpp; on split operands bit-identical to form 0) */
int sn_dbg_ref_block_f16_n(sn_handle *h, int n, const float *in, int h_px, int w, const float *w1, const float *b1,
                           const float *w2, const float *b2, int dil, int form, float *out);
int sn_dbg_ref_block_f16x3_n(sn_handle *h, int n, const float *in, int h_px, int w, const float *w1, const float *b1,
                             const float *w2, const float *b2, int dil, int form, float *out);
/* The LAST residual block of the fp16 tower followed by the refinement head (conv 3x3 32 -> 1, disp = relu(up + D r), wire
 * quantisation) on n images: fp32 host tensors in [n][32][hk][wk] (the level's padded activation, rounded to fp16 by the hook),
 * low [n][hk / ups][wk / ups] (the map the level starts from; ups = 16: soft-argmin map, 2: the level below), head_w [32][9].
 * form 0 = streamed block + k_head_final_f16 (two launches), 1 = the tail form the pipeline runs (one launch, y never
 * written); out_disp / out_raw [n][h_out][w_out], h_out <= hk, w_out <= wk.  The two forms must agree bit for bit. */
int sn_dbg_ref_tail_f16(sn_handle *h, int n, const float *in, int hk, int wk, const float *w1, const float *b1,
                        const float *w2, const float *b2, const float *head_w, float head_b, const float *low, int ups,
                        float dnorm, int h_out, int w_out, int form, float *out_disp, int32_t *out_raw);
/* Mid-stage hooks: the kernels between the feature tower and the output maps, one at a time, on caller tensors and through the
 * launch code of the forward pass.  Every device output lies between guard bands of known bytes and starts as the 0xff pattern
 * (fp32 NaN / int32 -1: an element the kernel does not write shows); a changed band or a non-zero border of a padded layout
 * returns SN_ERR_DEVICE with a message.  n = pairs (images for the heads), Dl <= 16 planes, hl x wl the low-resolution map.
 *
 * sn_dbg_cost_volume: feat [2n][32][hl][wl] (left, right interleaved) -> out [n][Dl][32][hl][wl], the split-slot cost volume
 * read back as hi + lo / 2048.  form 0 = k_cost_slots (plain layout), 1 = k_cost_slots_pad (zero-bordered volume of n pairs). */
int sn_dbg_cost_volume(sn_handle *h, const float *feat, int n, int Dl, int hl, int wl, int form, float *out);
/* the SN_PREC_FP32 first aggregation layer with the cost volume in its loader (LoadCostVol), LeakyReLU on:
 * wt [32][32][3][3][3], out [n][Dl][32][hl][wl] */
int sn_dbg_agg_first_f32(sn_handle *h, const float *feat, int n, int Dl, int hl, int wl, const float *wt, const float *bias,
                         float *out);
/* the soft-argmin alone.  form 0 = k_head_softargmin on v = a volume [n][Dl][32][hl][wl] with w [32][27] (ci, dz*9+ky*3+kx);
 * form 1 = k_softargmin_p on v = partial sums P [n][Dl][27][hl][wl] (w unused).  -> cost [n][Dl][hl][wl], disp_low [n][hl][wl],
 * conf_low [n][hl][wl] (written when want_conf; nullable otherwise, left as the 0xff pattern) and the count of pixels with a
 * non-finite cost. */
int sn_dbg_softargmin(sn_handle *h, int n, int Dl, int hl, int wl, int form, int want_conf, float bias, const float *v,
                      const float *w, float *cost, float *disp_low, float *conf_low, unsigned long long *nonfinite);
/* the LAST aggregation layer (fp32 output, LeakyReLU) of the fp16 modes followed by the soft-argmin, n pairs in one volume:
 * vol [n][32][Dl][hl][wl], wt [32][32][3][3][3], out_w [32][27].  form 0 = plain slots, k_conv_x3s (fp32 output) +
 * k_head_softargmin; 1 = zero-bordered slots, k_agg_x3s_dma<false> + k_head_softargmin; 2 = k_agg_x3s_dma<false, true>
 * (partial sums P) + k_softargmin_p.  layer_vol (nullable; forms 0 and 1 only): the layer's volume [n][Dl][32][hl][wl]. */
int sn_dbg_agg_tail(sn_handle *h, const float *vol, int n, int Dl, int hl, int wl, const float *wt, const float *bias,
                    const float *out_w, float out_b, int form, int want_conf, float *cost, float *disp_low, float *conf_low,
                    unsigned long long *nonfinite, float *layer_vol);
/* the refinement head alone on x [n][32][hk][wk] (the tower's output), arguments as sn_dbg_ref_tail_f16.  form 0 = k_head_final,
 * 1 = k_head_final_mfma32 (both need an SN_PREC_FP32 engine), 2 = the split head of SN_PREC_F16X3 on the hi / lo tensor (needs an
 * engine in an fp16 mode); SN_ERR_ARG with a message otherwise.  -> out_disp / out_raw [n][h_out][w_out], the mean |D r| per
 * written pixel (the refinement statistic) and the count of non-finite pixels. */
int sn_dbg_head(sn_handle *h, int n, const float *x, int hk, int wk, const float *head_w, float head_b, const float *low, int ups,
                float dnorm, int h_out, int w_out, int form, float *out_disp, int32_t *out_raw, double *mean_abs_dr,
                unsigned long long *nonfinite);
/* the image pyramid of the hierarchical refinement: in6 int8 [n][6][h][w] -> the float levels 1 .. levels - 1 one after the
 * other, level k [n][3][hp >> k][wp >> k] (hp / wp = ceil16), level 1 from the int8 input, the others from the level above */
int sn_dbg_img_pool2(sn_handle *h, const int8_t *in6, int n, int h_px, int w, int levels, float *out);
/* intermediates of the most recent batch-1 inference: "feat_l" / "feat_r" [32][hl][wl],
 * "cost" [Dl][hl][wl], "disp_low" [hl][wl], and for a hierarchical model "level1" .. "level3" (the map of that
 * refinement level, [Hp/2^k][Wp/2^k]); returns the element count in *n (dst may be NULL to query).
 * "conf_low" [hl][wl] is the confidence plane of the first pair of the most recent sn_infer_conf and meaningful only after
 * one: no other call writes it, so it reads zeros before the first sn_infer_conf and, after a later sn_infer, still that
 * earlier call's plane. */
int sn_dbg_read(sn_handle *h, const char *what, float *dst, size_t cap, size_t *n);
/* Parse()'s dequantisation + depth (stereonet_infer/src/parser.cpp:84-86) on the GPU, for n maps of the model's size:
 *     dis = (float)raw * out_scale;   depth_m = (float)((double)(focal_px * baseline_mm) / (dis * 16.0 * 12.0) / 1000.0)
 * with the reference's float / double mix, so the result is bit-identical to the host Parse (raw = 0 gives IEEE inf).
 * The reference's constants are focal_px = 527.1931762695312, baseline_mm = 119.89382172 (parser.cpp:70-71).
 * raw / depth_m: host or device buffers per `mem`; disp_px (nullable) receives dis * 16 * 12 as Parse's disparity. */
int sn_depth_from_raw(sn_handle *h, int n, const int32_t *raw, float focal_px, float baseline_mm, float *depth_m,
                      float *disp_px, int mem, void *stream);

/* ---- point cloud from the int32 map (what a sensor_msgs/PointCloud2 carries) --------------------------------------------
 * Camera of the rectified left eye, in pixels of the model's W x H map. */
typedef struct sn_camera {
  float fx, fy, cx, cy;   /* pinhole intrinsics                                                                     */
  float baseline_mm;      /* as sn_depth_from_raw (the reference's 119.89382172)                                    */
  float z_min_m, z_max_m; /* keep points with z_min_m <= Z <= z_max_m; z_max_m <= 0: no upper bound                 */
  int step;               /* 1, 2 or 4: every step-th row and column from 0; Ho = ceil(H/step), Wo = ceil(W/step)    */
} sn_camera;
enum { SN_PC_ORGANISED = 0, SN_PC_COMPACT = 1 };
/* n maps raw [n][H][W] -> points, 16 bytes {X, Y, Z, rgb} per point (`points` 16-byte aligned).  For output sample (i, j),
 * u = j*step, v = i*step, r = raw[k][v][u]:
 *   Z = sn_depth_from_raw's depth with focal_px = fx (the same float / double mix, bit for bit):
 *       Z = (float)((double)(fx * baseline_mm) / ((double)((float)r * out_scale) * 16.0 * 12.0) / 1000.0)
 *   X = ((float)u - cx) * Z / fx,  Y = ((float)v - cy) * Z / fy   (fp32, left to right, every step rounded, no FMA)
 *   valid: r > 0 && z_min_m <= Z && (z_max_m <= 0 || Z <= z_max_m)
 *   rgb: 0 without colour (nv12 == NULL); else the PCL packing 0x00RRGGBB of NV12 frame k.  nv12 holds n frames of
 *       F = nv12_pitch*(H + ceil(H/2)) bytes each (H luma rows, then ceil(H/2) interleaved chroma rows; for an even H that
 *       is nv12_pitch*H*3/2), frame k at nv12 + k*F (luma pitch nv12_pitch: W for a plain left image, 2W for FeedImg's
 *       side-by-side frame, whose left eye is the left half of every row), uv = frame + nv12_pitch*H,
 *       Y = y[v*pitch + u], U = uv[(v>>1)*pitch + (u&~1)], V = the byte after it (true NV12), and JFIF full-range BT.601
 *       in integers (>> arithmetic, clamp to 0..255): Uc = U-128, Vc = V-128,
 *       R = clamp(Y + ((91881*Vc + 32768) >> 16)), G = clamp(Y + ((-22554*Uc - 46802*Vc + 32768) >> 16)),
 *       B = clamp(Y + ((116130*Uc + 32768) >> 16))
 * SN_PC_ORGANISED: points [n][Ho][Wo][4]; an invalid sample is {0x7fc00000 x 3, 0} as bits; counts (nullable) [n] = valid
 *   samples per map.
 * SN_PC_COMPACT: map k's valid points in raster order from points + k*Ho*Wo*4, counts [n] (required) = how many; the
 *   words past the count are unspecified.
 * mem / stream as sn_depth_from_raw, except that a NULL stream is the point cloud's own stream (never the inference
 * stream); the call returns after completion when mem is SN_MEM_HOST or stream is NULL.  SN_ERR_ARG: n outside
 * 1..max_batch, a required pointer NULL, points misaligned, fx or fy <= 0 or not finite, baseline_mm <= 0, step not 1/2/4,
 * unknown layout, nv12 with nv12_pitch < W or odd.  SN_ERR_NOMEM: the scratch or the staging could not be allocated (as
 * in every other stage; earlier versions returned SN_ERR_DEVICE).
 * May run concurrently with sn_submit / sn_wait on the same handle: it has its own stream, scratch and staging (created
 * on first use, reused, freed by sn_destroy), and device-mode calls on different streams are ordered on that scratch by an
 * event. */
int sn_pointcloud_from_raw(sn_handle *h, int n, const int32_t *raw, const uint8_t *nv12, int nv12_pitch,
                           const sn_camera *cam, int layout, float *points, uint32_t *counts, int mem, void *stream);

/* ---- left-right consistency check: which pixels of the left map does the right eye confirm? --------------------------------
 * The network is left-referenced, so the right eye's map comes from the same weights: feed the mirrored pair (eyes swapped,
 * every row reversed) and reverse the rows of the result.  A left pixel is KEPT when the right map, sampled where the pixel's
 * own disparity sends it, holds the same disparity; occluded and out-of-view pixels do not.  A rejected pixel gets raw = 0,
 * which sn_depth_from_raw, sn_pointcloud_from_raw and Parse already read as "no measurement". */
typedef struct sn_lrc_params {
  float tau_px;         /* >= 0, finite: absolute tolerance in full-resolution pixels                    */
  float tau_rel;        /* >= 0, finite: plus this fraction of the left disparity (0 = absolute only)    */
  int   right_mirrored; /* sn_lr_check only: raw_right is stored column-reversed (the map of the mirrored
                           pair exactly as the network wrote it); 0 = right-image coordinates            */
} sn_lrc_params;
enum { SN_LRC_KEPT = 0, SN_LRC_INVALID_IN = 1, SN_LRC_OUT_OF_VIEW = 2, SN_LRC_NO_PARTNER = 4, SN_LRC_INCONSISTENT = 8 };
enum { SN_LRC_IN_TENSOR = 0, SN_LRC_IN_SBS_NV12 = 1 };
/* Common to the three functions: mem / stream as sn_infer_batch (NULL stream = the handle's own stream and the call returns
 * after completion; device buffers + a caller stream = work is only enqueued), calls on one handle must not overlap, n in
 * 1..max_batch.  SN_ERR_ARG: a required pointer NULL, a negative or non-finite tau_*, an unknown in_kind.  Their device
 * buffers (mirrored tensor, second map, copies of host data) are created on first use, only ever grown and freed by
 * sn_destroy.  Not covered: the asynchronous sn_submit* slots.
 *
 * sn_mirror_pair_i8: n model inputs [n][6][H][W] -> out[k][c][v][u] = in[k][(c + 3) % 6][v][W - 1 - u] (eyes swapped, rows
 *   reversed).  in and out must not overlap (SN_ERR_ARG).
 *
 * sn_lr_check: per map k, row v, column u, in fp32 with every operation rounded (no FMA contraction).  With
 *   S = (float)((double)out_scale * 192.0) and R(x) = raw_right[k][v][x] (raw_right[k][v][W - 1 - x] if right_mirrored):
 *     1. rl = raw_left[k][v][u];  rl <= 0 -> SN_LRC_INVALID_IN
 *     2. d = (float)rl * S;  xr = (float)u - d;  xr < 0 -> SN_LRC_OUT_OF_VIEW
 *     3. x0 = floor(xr), t = xr - (float)x0, x1 = min(x0 + 1, W - 1), r0 = R(x0), r1 = R(x1), d0 = (float)r0 * S,
 *        d1 = (float)r1 * S;  r0 <= 0 and r1 <= 0 -> SN_LRC_NO_PARTNER;  exactly one > 0: dr = its disparity;
 *        else dr = d0 + t * (d1 - d0)   (sub, mul, add, each rounded)
 *     4. !(fabsf(d - dr) <= tau_px + tau_rel * d) -> SN_LRC_INCONSISTENT
 *     5. otherwise SN_LRC_KEPT.  The first reason that applies wins.
 *   mask (nullable) [n][H][W] = the reason;  out_raw (nullable; out_raw == raw_left allowed) = rl where kept, 0 elsewhere;
 *   disp_inout (nullable) float [n][H][W]: 0.0f is written at exactly the rejected pixels, nothing else is touched;
 *   kept (nullable) [n] = kept pixels per map (integer sums: deterministic).  At least one of out_raw and mask is required;
 *   raw_right must not alias an output.
 *
 * sn_infer_lrc = L = sn_infer_batch(in);  M = sn_infer_batch(sn_mirror_pair_i8(in));  sn_lr_check(L, M, right_mirrored = 1), in
 *   the arithmetic the handle runs (two calls for sn_get_refine_stats; under SN_PREC_AUTO each forward follows the usual rule).
 *   out_i32 / out_disp (each nullable, not both) = the masked left map;  out_right_i32 (nullable) = M[..][W - 1 - x], the
 *   right eye's own disparity map in right-image coordinates, unmasked;  p->right_mirrored is ignored.
 *   in_kind SN_LRC_IN_TENSOR: in = int8 [n][6][H][W], w2 / h_px ignored;  SN_LRC_IN_SBS_NV12: in = n side-by-side NV12 frames as
 *   sn_preprocess_sbs_nv12_batch takes them (w2 = 2W, h_px = H, the same geometry restrictions and SN_ERR_ARG). */
int sn_mirror_pair_i8(sn_handle *h, int n, const int8_t *in_nchw6, int8_t *out_nchw6, int mem, void *stream);
int sn_lr_check(sn_handle *h, int n, const int32_t *raw_left, const int32_t *raw_right, const sn_lrc_params *p,
                int32_t *out_raw, float *disp_inout, uint8_t *mask, uint32_t *kept, int mem, void *stream);
int sn_infer_lrc(sn_handle *h, int n, const void *in, int in_kind, int w2, int h_px, const sn_lrc_params *p,
                 int32_t *out_i32, float *out_disp, int32_t *out_right_i32, uint8_t *mask, uint32_t *kept,
                 int mem, void *stream);

/* ---- confidence: how much of a pixel's matching distribution lies under the disparity it reports? ---------------------------
 * The soft-argmin holds the whole matching distribution of a low-resolution pixel and reports its expectation.  Whether that
 * expectation summarises one peak or averages two far-apart ones is the confidence; unlike the left-right check it costs no
 * second forward pass.
 *
 * Low resolution, per pair and per pixel of the hl x wl grid (hl = Hp / 16, wl = Wp / 16, Dl = D / 16).  With cost[d],
 *   m = max_d -cost[d], e_d = expf(-cost[d] - m), se = sum e_d, sd = sum d * e_d and dhat = sd / se exactly what the soft-argmin
 *   computes (dhat is the float it stores as its low-resolution disparity):
 *     Dl == 1 (D = 16): conf_low = 1.0f
 *     otherwise         k = min((int)floorf(dhat), Dl - 2);  conf_low = (e_k + e_{k+1}) / se
 *   — the probability mass on the two planes that bracket the expectation.  A single peak gives 1, and so does a peak shared by
 *   two neighbouring planes (an honest sub-plane disparity); two peaks j >= 2 planes apart give about the mass that happens to
 *   lie under their mean; a flat distribution gives 2 / Dl.  dhat lies in [0, Dl - 1], so k is always a valid plane.
 * Full resolution: conf[y][x] = the bilinear x16 upsample of conf_low (half-pixel centres, edge clamp: align_corners = False)
 *   for y < H, x < W — the function and the convention that feed the refinement its disparity, with factor 1 on the values, and
 *   the same for single-scale and hierarchical models (the confidence describes the cost volume).  The sample positions are
 *   multiples of 1/32: the bilinear weights are exact in fp32.
 * Mask, per pixel, with r = raw[k][v][u] and c = conf[k][v][u]:
 *     1. r <= 0              -> SN_CONF_INVALID_IN (1)
 *     2. !(c >= min_conf)    -> SN_CONF_LOW (64): a NaN confidence is rejected at every threshold
 *     3. otherwise kept (0).
 *   64 is disjoint from the SN_LRC_* bits (1, 2, 4, 8) and the SN_FLT_* bits (16, 32): masks can be OR-ed.
 *   Outputs as sn_lr_check's: out_raw (out_raw == raw allowed) = r where kept, 0 elsewhere; disp_inout gets 0.0f at exactly
 *   the rejected pixels, nothing else is touched; kept[n] = kept pixels per map (integer sums: deterministic). */
typedef struct sn_conf_params { float min_conf; } sn_conf_params;   /* 0..1, finite; 0 rejects only NaN */
enum { SN_CONF_KEPT = 0, SN_CONF_INVALID_IN = 1, SN_CONF_LOW = 64 };
/* sn_infer_conf: ONE forward pass (one call for sn_get_refine_stats; under SN_PREC_AUTO a blocking call follows the usual
 *   rule, and a repeated call's outputs all belong to the arithmetic that returned).  in / in_kind / w2 / h_px / mem / stream /
 *   blocking / n in 1..max_batch exactly as sn_infer_lrc (SN_LRC_IN_TENSOR, SN_LRC_IN_SBS_NV12); the NULL stream is the
 *   handle's inference stream.  out_i32 / out_disp (each nullable, not both) = the map, masked when p is given;
 *   out_conf (nullable) float [n][H][W] = conf;  p == NULL: no masking — the outputs are the plain map of sn_infer_batch plus
 *   out_conf, and mask and kept must then be NULL;  mask (nullable) [n][H][W], kept (nullable) [n] as above.
 * sn_conf_mask: stateless — the mask rules on any map raw [n][H][W] of the model's size and a full-resolution conf [n][H][W]
 *   (that of sn_infer_conf, also after sn_lr_check or sn_filter_raw have worked on the map).  At least one of out_raw and mask
 *   is required.
 * SN_ERR_ARG: a required pointer NULL, min_conf outside [0, 1] or not finite, an unknown in_kind, an image size that does not
 *   match the model input, n outside 1..max_batch, conf overlapping an output.  Device buffers (copies of host data, the map the
 *   rules read when the caller asks for the float map alone) are shared with the left-right check: created on first use, only
 *   ever grown, freed by sn_destroy; calls on one handle must not overlap.  Not covered: the asynchronous sn_submit* slots and
 *   the node. */
int sn_infer_conf(sn_handle *h, int n, const void *in, int in_kind, int w2, int h_px, const sn_conf_params *p,
                  int32_t *out_i32, float *out_disp, float *out_conf, uint8_t *mask, uint32_t *kept,
                  int mem, void *stream);
int sn_conf_mask(sn_handle *h, int n, const int32_t *raw, const float *conf, const sn_conf_params *p,
                 int32_t *out_raw, float *disp_inout, uint8_t *mask, uint32_t *kept, int mem, void *stream);

/* ---- speckle removal and hole filling of the int32 map: what a consistency check leaves behind ---------------------------------
 * sn_infer_lrc zeroes what the right eye does not confirm.  Two things remain: SPECKLES, small islands of surviving pixels
 * (and small patches whose disparity is unlike everything around them), and HOLES, the occlusion strip behind a foreground
 * edge and single rejected pixels.  sn_filter_raw removes the first and fills the second, on the GPU, in integers. */
typedef struct sn_filter_params {
  int   speckle_max_px;   /* 0: no speckle removal; else 1..H*W: components of at most this many pixels are removed */
  float speckle_diff_px;  /* >= 0, finite: 4-neighbours belong together when their disparities differ by at most this */
  int   fill_max_px;      /* 0: no filling; else >= 1: row gaps of at most this many pixels are filled */
} sn_filter_params;
enum { SN_FLT_INVALID_IN = 1, SN_FLT_SPECKLE = 16, SN_FLT_FILLED = 32 };   /* bits; 0 = untouched measurement */
/* sn_filter_raw: n maps raw [n][H][W] of the model's size, each on its own.  All per-pixel arithmetic is integer.  With
 *   S = (float)((double)out_scale * 192.0) as for sn_lr_check, the link threshold in units of raw is
 *   dq = (int64_t)floorf(speckle_diff_px / S), one fp32 division on the host (a quotient of 2^32 or more is taken as 2^32: two
 *   int32 values never differ by that much).
 *   Stage 1, speckles (speckle_max_px > 0).  A pixel is valid when raw > 0.  Two 4-neighbours a, b are LINKED when both are
 *     valid and |(int64_t)a - (int64_t)b| <= dq (64 bits: INT32_MAX beside 1 does not wrap).  The components are the connected
 *     components of that graph, an equivalence relation, so nothing depends on the order of traversal.  Every pixel of a
 *     component of at most speckle_max_px pixels gets the value 0 and the bit SN_FLT_SPECKLE.  (OpenCV's filterSpeckles:
 *     4-connectivity, <= maxDiff, <= maxSpeckleSize.)  M = the map after this stage (raw <= 0 counts as 0).
 *   Stage 2, fill (fill_max_px > 0), per row v.  For a column u with M[v][u] <= 0: ul = the nearest column left of u with
 *     M > 0, ur = the nearest to the right.  Neither exists: the pixel is untouched.  Otherwise
 *     gap = (ur or W) - (ul or -1) - 1, and if gap <= fill_max_px the pixel takes min(M[v][ul], M[v][ur]) — the smaller
 *     disparity is the background, which is what an occlusion hides — or the one bounding value where the gap touches an
 *     image border, and the bit SN_FLT_FILLED.  Sources are pixels of M only, never filled values: rows are independent.
 *   mask (nullable) [n][H][W] = OR of the bits, SN_FLT_INVALID_IN where raw <= 0: one of 0, 1, 16, 33, 48; the result is > 0
 *     exactly where mask == 0 or SN_FLT_FILLED is set.
 *   out_raw (nullable) = the final value, 0 at every pixel that ends invalid (a negative input becomes 0); out_raw == raw is
 *     allowed, any other overlap between the buffers is SN_ERR_ARG.
 *   disp_inout (nullable) float [n][H][W]: where mask != 0, 0.0f if the pixel ends invalid, else (float)value * S (one rounded
 *     multiply); nothing else is touched.
 *   counts (nullable) [n][3] = {pixels with result > 0, with SN_FLT_SPECKLE, with SN_FLT_FILLED} per map (integer sums:
 *     deterministic).  At least one of out_raw and mask is required.
 * SN_ERR_ARG: n outside 1..max_batch, p or raw NULL, speckle_max_px outside 0..H*W, speckle_diff_px negative or not finite,
 * fill_max_px < 0, both stages off, neither out_raw nor mask, overlapping buffers.
 * mem / stream as sn_pointcloud_from_raw: a NULL stream is the filter's own stream (never the inference stream); the call
 * returns after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller stream only enqueue.  May run
 * concurrently with sn_submit / sn_wait on the same handle: stream, scratch and staging are its own (created on first use,
 * reused, freed by sn_destroy), and calls on different streams are ordered on the scratch by an event.  The scratch (a label
 * and a size, 8 bytes per pixel) holds min(max_batch, 8) maps; a larger n is walked in slices of 8 maps on the stream.
 * Not covered: the asynchronous sn_submit* slots. */
int sn_filter_raw(sn_handle *h, int n, const int32_t *raw, const sn_filter_params *p, int32_t *out_raw,
                  float *disp_inout, uint8_t *mask, uint32_t *counts, int mem, void *stream);

/* ---- guided weighted-median smoothing of the int32 map: the edge-preserving smoother after check, filter and confidence -------
 * sn_filter_raw fills every row on its own, which leaves streaks behind a foreground edge; isolated outliers of the soft-argmin
 * pass the left-right check and are too well connected to be speckles; the refinement's sub-pixel noise roughens every surface
 * of the point cloud.  A median removes all three but rounds corners and thin structures; a median WEIGHTED by the similarity
 * of the left image's luma does not.  sn_smooth_raw computes it on the GPU, in integers. */
typedef struct sn_smooth_params {
  int radius;      /* 1, 2 or 3: the window is (2*radius+1)^2, clipped to the image (no padding)            */
  int sigma_luma;  /* 0: plain median, guide ignored (may be NULL); 1..255: weight falls with |luma diff|  */
  int min_valid;   /* 0: a pixel without a measurement stays without one; 1..(2*radius+1)^2: it takes the  */
                   /* window's weighted median when at least this many window pixels hold a measurement    */
} sn_smooth_params;
enum { SN_SMOOTH_INVALID_IN = 1, SN_SMOOTH_CHANGED = 128 };   /* 128: the last free bit beside SN_LRC_*, SN_FLT_*, SN_CONF_LOW */
enum { SN_GUIDE_NV12 = 0, SN_GUIDE_TENSOR = 1 };
/* sn_smooth_raw: n maps raw [n][H][W] of the model's size, each on its own.  All per-pixel arithmetic is integer.
 *   Luma Y(k, v, u), 0..255, of map k's left image:
 *     SN_GUIDE_NV12: the luma byte of frame k, guide + k*F + v*guide_pitch + u, with the layout, the frame stride
 *       F = guide_pitch*(H + ceil(H/2)) and guide_pitch exactly as sn_pointcloud_from_raw's nv12 / nv12_pitch (W for a plain
 *       left image, 2W for FeedImg's side-by-side frame).  Only the luma rows are read.
 *     SN_GUIDE_TENSOR: guide is the int8 model input [n][6][H][W] and Y = (uint8_t)guide[k][0][v][u] ^ 0x80; guide_pitch is
 *       ignored.
 *   Weight table, computed once on the host: T[j] = 1 for every j when sigma_luma == 0 (the guide is not read); otherwise, with
 *     s = sigma_luma, T[j] = (256*s*s) / (s*s + j*j) in integer division for j = 0..255 — a Lorentzian, T[0] = 256, and it may
 *     reach 0.
 *   Per pixel p = (v, u): the PARTICIPANTS are the pixels q of the window around p that lie inside the image, have raw[q] > 0
 *     and a weight w_q = T[|Y(q) - Y(p)|] > 0.  Wt = the sum of w_q over the participants.  The weighted median is
 *       m = min{ raw[q] : 2 * (sum of w_q' over the participants q' with raw[q'] <= raw[q]) >= Wt }
 *     — the LOWER weighted median: it depends on no traversal or tie order and is always the value of a participant.
 *   Result:  raw[p] > 0: m (the centre takes part with weight T[0] > 0, so m exists).
 *            raw[p] <= 0: m if min_valid > 0, at least min_valid pixels of the window have raw > 0 (counted regardless of
 *            their weight) and Wt > 0; otherwise 0.
 *   mask (nullable) [n][H][W] = SN_SMOOTH_INVALID_IN where raw <= 0, OR SN_SMOOTH_CHANGED where the result differs from
 *     max(raw, 0): one of 0, 1, 128, 129; the result is > 0 exactly where mask is 0, 128 or 129.  128 is disjoint from the
 *     SN_LRC_* bits (1, 2, 4, 8), the SN_FLT_* bits (16, 32) and SN_CONF_LOW (64): masks can be OR-ed.
 *   out_raw (nullable) = the result; out_raw == raw is allowed (the call then reads a copy of the map in its scratch, never
 *     what it has already overwritten), any other overlap between the buffers is SN_ERR_ARG, and the guide must not overlap an
 *     output.
 *   disp_inout (nullable) float [n][H][W]: where SN_SMOOTH_CHANGED is set, 0.0f if the result is 0, else (float)result * S with
 *     S = (float)((double)out_scale * 192.0) (one rounded multiply); nothing else is touched — sn_filter_raw's rule.
 *   counts (nullable) [n][3] = {pixels with result > 0, changed with raw > 0, changed with raw <= 0} per map (integer sums:
 *     deterministic).  At least one of out_raw and mask is required.
 * SN_ERR_ARG: n outside 1..max_batch, p or raw NULL, radius outside 1..3, sigma_luma outside 0..255, sigma_luma > 0 with guide
 * NULL, an unknown guide_kind, SN_GUIDE_NV12 with guide_pitch < W or odd, min_valid outside 0..(2*radius+1)^2, neither out_raw
 * nor mask, overlapping buffers.
 * mem / stream as sn_filter_raw: a NULL stream is the smoother's own stream (never the inference stream); the call returns
 * after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller stream only enqueue.  May run
 * concurrently with sn_submit / sn_wait on the same handle: stream, scratch and staging are its own (created on first use,
 * only ever grown, freed by sn_destroy), and calls on different streams are ordered on the scratch by an event.  The scratch
 * (the copy an in-place call reads, 4 bytes per pixel) holds min(max_batch, 8) maps; a larger n is walked in slices of 8 maps
 * on the stream.  Not covered: the asynchronous sn_submit* slots and the node. */
int sn_smooth_raw(sn_handle *h, int n, const int32_t *raw, const void *guide, int guide_kind, int guide_pitch,
                  const sn_smooth_params *p, int32_t *out_raw, float *disp_inout, uint8_t *mask, uint32_t *counts,
                  int mem, void *stream);

/* ---- temporal filter of disparity STREAMS: the one stage of the chain that keeps state between calls --------------------------
 * Every stage above treats a map on its own.  A learned matcher shows its noise over time: surfaces shimmer from frame to
 * frame, and pixels that the check or the confidence mask reject flicker in and out.  sn_temporal blends a pixel with its own
 * filtered past while it stays near it, holds the last value over short dropouts, and lets go at once where the left image's
 * luma says that the scene moved.  Integer per pixel and bit-exact; the state lives on the GPU, one set per stream. */
typedef struct sn_temporal_params {
  int   alpha;       /* 1..256: the weight of the new measurement in 1/256; 256 = no blending                       */
  float delta_px;    /* >= 0, finite: blend only while |new - last| <= this many pixels                             */
  int   persist;     /* 0: never fill; 1..8: a pixel without a measurement keeps its last value while at least this */
                     /* many of its last eight inputs held one                                                      */
  int   luma_delta;  /* 0: the guide is not read (may be NULL); 1..255: a luma change above this counts as motion   */
} sn_temporal_params;
/* The eight bits of the chain's OR-able mask are all taken (SN_LRC_* 1 2 4 8, SN_FLT_* 16 32, SN_CONF_LOW 64,
 * SN_SMOOTH_CHANGED 128), so the temporal mask is a PLANE OF ITS OWN with its own enum: it must not be OR-ed with the others. */
enum { SN_TMP_INVALID_IN = 1, SN_TMP_BLENDED = 2, SN_TMP_HELD = 4, SN_TMP_MOVED = 8, SN_TMP_JUMP = 16 };
typedef struct sn_temporal sn_temporal;
/* With S = (float)((double)out_scale * 192.0) as for sn_filter_raw, q = (int64_t)floorf(delta_px / S), one fp32 division on
 *   the host (a quotient of 2^32 or more is taken as 2^32), exactly as sn_filter_raw turns speckle_diff_px into dq.
 * State per stream and pixel (6 bytes): P int32 >= 0, the last filtered value, 0 = none; Hs uint8, bit i = the input i + 1
 *   frames ago held a measurement; Yp uint8, the last frame's luma.  A fresh or reset stream has P = 0, Hs = 0 and has seen no
 *   frame (there is no previous luma).
 * One frame of a stream, per pixel, with r = max(raw, 0) and y = the left image's luma Y(k, v, u) — guide, guide_kind and
 *   guide_pitch exactly as sn_smooth_raw's (SN_GUIDE_NV12 with the frame stride and pitch rules of sn_pointcloud_from_raw,
 *   SN_GUIDE_TENSOR); with luma_delta == 0 the guide is not read:
 *     moved = luma_delta > 0 && the stream has seen a frame && |y - Yp| > luma_delta
 *     r > 0:   P > 0 && !moved && |r - P| <= q (in 64 bits):
 *                  out = (alpha*r + (256 - alpha)*P + 128) >> 8 in 64 bits (never 0: r, P >= 1), SN_TMP_BLENDED if out != r;
 *              otherwise out = r, and where P > 0: SN_TMP_MOVED if moved, else SN_TMP_JUMP.
 *              P' = out.
 *     r == 0:  SN_TMP_INVALID_IN, and
 *              persist > 0 && P > 0 && !moved && popcount(Hs) >= persist: out = P, SN_TMP_HELD, P' = P;
 *              otherwise out = 0; P > 0 && moved: SN_TMP_MOVED and P' = 0; else P' = P.
 *     then Hs' = ((Hs << 1) | (r > 0)) & 255, and Hs' == 0 sets P' = 0: a held value is never older than eight frames;
 *     then Yp' = y.
 *   The mask is one of 0, 1, 2, 5, 8, 9, 16; out > 0 exactly where it is 0, 2, 5, 8 or 16.
 * sn_temporal_create: a filter of `streams` independent states (1 <= streams <= max_batch) on handle h, all fresh; the state
 *   (6 * H * W * streams bytes), a stream, an event and the host-mode staging are the object's own.  SN_ERR_ARG: a NULL pointer,
 *   streams out of range, alpha outside 1..256, delta_px negative or not finite, persist outside 0..8, luma_delta outside
 *   0..255.  While a filter is alive sn_destroy(h) is REFUSED: it returns SN_ERR_BUSY and leaves the handle as it was — destroy
 *   the handle's filters first.
 * sn_temporal_reset: stream `stream` (-1: all) is fresh again.  A host-side flag that takes effect at the next push: no device
 *   work, no memset, nothing to order.  SN_ERR_ARG: an id outside -1..streams-1.
 * sn_temporal_push: n maps raw [n][H][W] (1 <= n <= max_batch); map k is the next frame of stream stream_of[k] (a host array
 *   of n ids; NULL: every map belongs to stream 0, i.e. the call is one clip).  Maps with the same id are consecutive frames in
 *   the order of k, and the result equals n single-map pushes in that order, bit for bit.
 *   out_raw (nullable) = out; out_raw == raw is allowed (the kernel is pointwise: no copy), any other overlap between the
 *     buffers is SN_ERR_ARG, and the guide must not overlap an output.
 *   mask (nullable) [n][H][W] = the bits above.  At least one of out_raw and mask is required.
 *   disp_inout (nullable) float [n][H][W]: rewritten exactly where out != r, as (float)out * S (one rounded multiply,
 *     sn_filter_raw's rule; out > 0 there); nothing else is touched.
 *   counts (nullable) [n][4] = {pixels with out > 0, with SN_TMP_BLENDED, with SN_TMP_HELD, with SN_TMP_MOVED or SN_TMP_JUMP}
 *     per map (integer sums: deterministic).
 *   SN_ERR_ARG (sn_last_error(h) names the call; nothing is launched and no state changes): n out of range, raw NULL, neither
 *     out_raw nor mask, an id outside 0..streams-1, luma_delta > 0 with guide NULL, an unknown guide_kind, SN_GUIDE_NV12 with
 *     guide_pitch < W or odd, overlapping buffers, a bad mem.
 *   mem / stream as sn_filter_raw: a NULL stream is the filter's own stream (never the inference stream); the call returns
 *   after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller stream only enqueue.  May run beside
 *   sn_submit / sn_wait on the same handle, and calls are serialised by the object's mutex; pushes on different streams are
 *   ordered on the state by an event.  One kernel launch per 64 maps of a call.  Not covered: the asynchronous sn_submit* slots. */
int  sn_temporal_create(sn_handle *h, int streams, const sn_temporal_params *p, sn_temporal **out);
int  sn_temporal_reset(sn_temporal *t, int stream);
void sn_temporal_destroy(sn_temporal *t);
int  sn_temporal_push(sn_temporal *t, int n, const int *stream_of, const int32_t *raw, const void *guide, int guide_kind,
                      int guide_pitch, int32_t *out_raw, float *disp_inout, uint8_t *mask, uint32_t *counts, int mem,
                      void *stream);

/* ---- stereo rectification from the camera calibration: the head of the chain ----------------------------------------------------
 * Every stage above assumes a RECTIFIED pair: undistorted, row-aligned and exactly the model's W x H.  sn_rectify makes one
 * from raw NV12 frames of any source size and a calibration in the form a ROS CameraInfo pair or OpenCV's stereoRectify
 * delivers: K, D (plumb-bob k1 k2 p1 p2 k3) and R per eye and the common rectified projection P.  It writes the side-by-side
 * NV12 frame that sn_infer_sbs_nv12, sn_submit_nv12, sn_infer_lrc, the point cloud's colour and the guides take, optionally the
 * int8 model tensor, and hands back the sn_camera of the rectified left eye. */
typedef struct sn_eye_calib { double fx, fy, cx, cy; double d[5]; double R[9]; } sn_eye_calib;
typedef struct sn_stereo_calib {
  int src_w, src_h;                 /* one eye of the raw frame; both even, 2..8192                              */
  sn_eye_calib left, right;
  double pfx, pfy, pcx, pcy;        /* common rectified projection, in pixels of the model's W x H               */
  double baseline_mm;               /* > 0; passed through to sn_camera                                          */
} sn_stereo_calib;
typedef struct sn_rectify sn_rectify;
typedef struct sn_rectify_info { int src_w, src_h, w, h; uint32_t valid_left, valid_right; } sn_rectify_info;
/* Two stages with an exact interface between them, so that every comparison with the numpy twin
 * (hobot_stereonet_amd/rectify.py) is bit for bit.
 *
 * Stage A: the map.  Built once per calibration, on the host, in double.  For an eye with source intrinsics fx fy cx cy,
 * distortion k1 k2 p1 p2 k3 = d[0..4], rectifying rotation R (row-major, source camera to rectified camera) and the common
 * rectified projection pfx pfy pcx pcy, for every destination pixel (u, v), 0 <= u < W, 0 <= v < H, in exactly this order of
 * operations, every step one rounded IEEE operation, no FMA (sw x sh = src_w x src_h):
 *
 *   x = ((double)u - pcx) / pfx;            y = ((double)v - pcy) / pfy
 *   X = R[0]*x + R[3]*y + R[6];  Y = R[1]*x + R[4]*y + R[7];  Wc = R[2]*x + R[5]*y + R[8]     (R^T * [x y 1], left to right)
 *   if !(Wc > 0): sentinel
 *   a = X/Wc; b = Y/Wc; a2 = a*a; b2 = b*b; r2 = a2 + b2; ab2 = 2.0*(a*b)
 *   rad = 1.0 + r2*(k1 + r2*(k2 + r2*k3))
 *   xd = a*rad + (p1*ab2 + p2*(r2 + 2.0*a2));      yd = b*rad + (p1*(r2 + 2.0*b2) + p2*ab2)
 *   us = fx*xd + cx;  vs = fy*yd + cy
 *   if !(us > -1 && us < sw && vs > -1 && vs < sh): sentinel         (NaN fails the test: sentinel)
 *   mx = (int32)floor(us*256.0 + 0.5);  my = (int32)floor(vs*256.0 + 0.5)
 *
 * The map is int32 [H][W][2] = (mx, my), in units of 1/256 source pixel.  Integer coordinates are pixel centres (OpenCV's
 * convention).  The sentinel is (INT32_MIN, INT32_MIN).
 *
 * Stage B: the remap.  Per frame, on the GPU, in integers.  With B the border value (0 for luma, 128 for chroma) and a source
 * plane of pw x ph samples:
 *
 *   sentinel            -> out = B
 *   x0 = mx >> 8 (arithmetic), y0 = my >> 8, fx = mx & 255, fy = my & 255
 *   p(i,j) = source sample at (x0+i, y0+j) if 0 <= x0+i < pw and 0 <= y0+j < ph, else B        (per tap)
 *   out = ((256-fx)*(256-fy)*p(0,0) + fx*(256-fy)*p(1,0) + (256-fx)*fy*p(0,1) + fx*fy*p(1,1) + 32768) >> 16
 *
 * Luma: the formula at every (u, v) on the sw x sh luma plane.  Chroma: true NV12, interleaved UV rows, W/2 x H/2 samples; for
 * chroma sample (cj, ci) take the luma map entry at (2cj, 2ci); if it is not the sentinel, (mx >> 1, my >> 1) is a Q8
 * coordinate on the sw/2 x sh/2 chroma plane, and U and V are blended separately with the same weights.  The identity
 * calibration gives mx = 256u, and the output equals the input byte for byte.
 *
 * sn_rectify_build_map: Stage A of eye `eye` (0 left, 1 right) for a w x h destination into map_xy [h][w][2].  Pure host: no
 *   device and no handle.  SN_ERR_ARG: a NULL pointer, an eye other than 0 or 1, w or h < 1, src_w or src_h odd or outside
 *   2..8192, a non-finite field, fx, fy (of either eye), pfx, pfy or baseline_mm <= 0.
 * sn_rectify_create: a rectifier for handle h's model size W x H.  The same checks, and W % 4 != 0 or an odd H is SN_ERR_ARG
 *   (sn_last_error(h) says so: the frames of such a model are not accepted by the side-by-side entry points either).  Both maps
 *   are built on the host and uploaded (2 * H * W * 8 bytes); a stream, an event, a mutex and the staging are the object's own.
 *   While a rectifier is alive sn_destroy(h) is REFUSED with SN_ERR_BUSY, as for sn_temporal.
 * sn_rectify_get_info: the sizes and valid_left / valid_right, the number of map entries that are not the sentinel.
 * sn_rectify_get_camera: {(float)pfx, (float)pfy, (float)pcx, (float)pcy, (float)baseline_mm, 0, 0, 1}.
 * sn_rectify_get_map: downloads the device copy of an eye's map into map_xy_host [H][W][2] (the maps never change after create).
 * sn_rectify_nv12: n raw pairs, 1 <= n <= max_batch.  Pair k's eyes are at left + k*src_frame and right + k*src_frame; each eye
 *   is an NV12 image of luma pitch src_pitch: src_h luma rows, then src_h/2 interleaved chroma rows of the same pitch.  A
 *   side-by-side camera frame is right = left + src_w with src_pitch >= 2*src_w; separate eyes are two buffers of pitch >=
 *   src_w.  Source pointers need no alignment.  src_pitch * src_h * 3/2 must be below 2^31.
 *   out_sbs_nv12 (nullable): [n] side-by-side frames of pitch 2W, 3*W*H bytes each.
 *   out_nchw6 (nullable): [n][6][H][W], sn_preprocess_sbs_nv12_batch's tensor of the rectified frame, written on the same
 *     stream (through the object's scratch when out_sbs_nv12 is NULL).  At least one of the two outputs is required;
 *     device-mode outputs must be 4-byte aligned.
 *   Overlap between any input span and any output span, or between the outputs, is SN_ERR_ARG.
 *   SN_ERR_ARG (sn_last_error(h) names the call; nothing is launched): n out of range, an input NULL, both outputs NULL,
 *     src_pitch < src_w, a frame too large, a misaligned device output, overlapping buffers, a bad mem.
 *   mem / stream as sn_temporal_push: a NULL stream is the rectifier's own stream (never the inference stream); the call
 *   returns after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller stream only enqueue.  May
 *   run beside sn_submit / sn_wait on the same handle; calls are serialised by the object's mutex, and calls on different
 *   streams are ordered on the scratch by an event.  One remap launch per call.  Not covered: the asynchronous sn_submit*
 *   slots, fisheye and rational distortion models, a principal point per eye (one pcx for both). */
int  sn_rectify_build_map(const sn_stereo_calib *c, int eye, int w, int h, int32_t *map_xy);
int  sn_rectify_create(sn_handle *h, const sn_stereo_calib *c, sn_rectify **out);
void sn_rectify_destroy(sn_rectify *r);
int  sn_rectify_get_info(const sn_rectify *r, sn_rectify_info *info);
int  sn_rectify_get_camera(const sn_rectify *r, sn_camera *cam);
int  sn_rectify_get_map(sn_rectify *r, int eye, int32_t *map_xy_host);
int  sn_rectify_nv12(sn_rectify *r, int n, const uint8_t *left, const uint8_t *right, int src_pitch, size_t src_frame,
                     uint8_t *out_sbs_nv12, int8_t *out_nchw6, int mem, void *stream);

/* ---- baseline JPEG of NV12 images: the left-eye picture of the node's message, on the GPU ----------------------------------------
 * For every frame sn_jpeg_encode_nv12 produces exactly the bytes of the host encoder EncodeNv12ToJpegSliced(nv12, w, h, pitch,
 * quality, rows_per_slice) of csrc/compat/src/jpeg_nv12.cpp.  No tolerance: the same bytes.  hobot_stereonet_amd/jpeg.py is the
 * numpy twin.  The contract:
 *
 *   Header: SOI, APP0 (JFIF 1.1), two DQT, SOF0 (8 bit; Y 2x2, Cb and Cr 1x1), four DHT with the ITU T.81 Annex K tables, DRI
 *     only when sliced, SOS: 623 bytes, 629 with DRI.
 *   Quality: clamped to 1..100; sf = quality < 50 ? 5000 / quality : 200 - 2 * quality; q = clamp((base * sf + 50) / 100, 1, 255).
 *   Samples: NV12 is the YCbCr 4:2:0 that the stream stores: (float)byte - 128.  MCUs of 16x16 pixels in raster order, blocks
 *     Y0 Y1 Y2 Y3 Cb Cr.  A block cut by the right or bottom edge replicates the last column or row of its plane; the chroma
 *     planes are w/2 x h/2 samples, read interleaved from the rows behind the luma rows.
 *   Transform: the AAN forward DCT in fp32, every operation rounded once, NO fused multiply-add, in this order: the 8-point pass
 *     down the columns, transpose, the same pass again (so coefficient (v, u) ends at [u][v]).  One pass, on d[0..7]:
 *       t0 = d0 + d7; t7 = d0 - d7; t1 = d1 + d6; t6 = d1 - d6; t2 = d2 + d5; t5 = d2 - d5; t3 = d3 + d4; t4 = d3 - d4
 *       e0 = t0 + t3; e3 = t0 - t3; e1 = t1 + t2; e2 = t1 - t2;  d0 = e0 + e1; d4 = e0 - e1
 *       z1 = (e2 + e3) * 0.707106781f;  d2 = e3 + z1; d6 = e3 - z1
 *       o0 = t4 + t5; o1 = t5 + t6; o2 = t6 + t7;  z5 = (o0 - o2) * 0.382683433f
 *       z2 = 0.541196100f * o0 + z5;  z4 = 1.306562965f * o2 + z5;  z3 = o1 * 0.707106781f
 *       z11 = t7 + z3; z13 = t7 - z3;  d5 = z13 + z2; d3 = z13 - z2; d1 = z11 + z4; d7 = z11 - z4
 *   Quantisation: lrintf(coefficient * recip), ties to even, recip = (float)(1.0 / (q * aan[u] * aan[v] * 8.0)) with
 *     aan = {1, 1.387039845, 1.306562965, 1.175875602, 1, 0.785694958, 0.541196100, 0.275899379}.
 *   Entropy coding: one DC predictor per component, reset at every slice; AC run / size symbols in zigzag order, ZRL (0xF0) for
 *     runs over 15, EOB unless coefficient 63 is non-zero.
 *   Slices: rows_per_slice MCU rows form a restart interval (DRI = rows_per_slice * ceil(w / 16) MCUs).  A slice ends with its
 *     last partial byte padded with ones; a zero byte is stuffed after every 0xFF.  FF D0+(k mod 8) follows slice k, FF D9 the
 *     last.  rows_per_slice <= 0 or >= ceil(h / 16): a single scan without DRI.
 *
 * sn_jpeg_bound: a capacity no stream of a w x h image can exceed (the header, 416 bytes per 8x8 block, the markers); 0 for a
 *   size the encoder does not take.  Pure host.
 * sn_jpeg_encode_nv12: n images (1 <= n <= max_batch) of w x h pixels, image k at nv12 + k * frame: h luma rows of `pitch`
 *   bytes, the h/2 chroma rows behind them at nv12 + h * pitch.  w and h are arguments, not the model's; any address and any
 *   pitch >= w: odd addresses, the left half of a side-by-side frame (pitch = 2w), what sn_rectify_nv12 wrote.
 *   Stream k goes to out + k * out_stride and its length to sizes[k].  A stream that does not fit out_stride gives sizes[k] = 0
 *   (no valid stream is shorter than its header) and not one byte of it is stored; the other frames of the call are
 *   unaffected, and the call returns SN_OK.  Nothing is ever written at or beyond out + (k + 1) * out_stride.
 *   SN_ERR_ARG (sn_last_error(h) says why; nothing is launched or written): a NULL pointer, n out of range, w or h odd or
 *     outside 2..65535, pitch < w, more than 65535 MCUs in a restart interval, an image so large that sn_jpeg_bound exceeds
 *     2^32 - 1, the images overlapping out or sizes, a bad mem.  SN_ERR_NOMEM: the scratch could not be allocated.
 *   mem / stream as sn_filter_raw: a lane of the handle's with a stream, an event and grow-only scratch of its own (never the
 *   inference stream); the call returns after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller
 *   stream only enqueue.  May run beside sn_submit / sn_wait and beside the other stages; calls are serialised by the lane's
 *   mutex.  The batch is walked eight frames at a time, so the scratch (128 bytes per block for the coefficients, 416 for the
 *   slices) does not grow with n.  Parallelism is n x slices: a single-scan stream is one sequential chain per frame, correct
 *   but slow; use rows_per_slice = 1 where the consumer accepts restart markers.  Not covered: the asynchronous sn_submit*
 *   slots, optimised Huffman tables, progressive or 4:4:4 streams, a decoder.
 * sn_dbg_jpeg_dct: the fp32 coefficients BEFORE quantisation of one host image, out [blocks][64] in coding order, coefficient
 *   (v, u) of a block at u * 8 + v: a contracted or reordered transform shows in the last bit of almost every value. */
typedef struct sn_jpeg_params { int quality; int rows_per_slice; } sn_jpeg_params;
size_t sn_jpeg_bound(int w, int h_px);
int  sn_jpeg_encode_nv12(sn_handle *h, int n, const uint8_t *nv12, int w, int h_px, int pitch, size_t frame,
                         const sn_jpeg_params *p, uint8_t *out, size_t out_stride, uint32_t *sizes, int mem, void *stream);
int  sn_dbg_jpeg_dct(sn_handle *h, const uint8_t *nv12, int w, int h_px, int pitch, float *out);

/* ---- the depth view: colour-mapped depth under the left eye, the picture of the reference's render node -------------------------
 * The reference's render node (MinimalPublisher.listener_callback) turns the int32 map into metric depth, applies
 * convertScaleAbs(alpha = 9) and COLORMAP_JET, stacks the result under the left image and publishes it as a JPEG.  sn_render
 * makes that canvas from the map and the left eye in device memory, sn_render_jpeg its JPEG.  No tolerance: the numpy twin
 * (hobot_stereonet_amd/render.py: canvas, canvas_jpeg), the host C++ twin (compat/src/render.cpp: RenderCanvas) and the kernel
 * give the same bytes.  Making the JET table or the final bytes match OpenCV's is not claimed (parity unpinned: no cv2 to diff).
 *
 * Colour index of a pixel with map word raw, viewed as uint32 as the reference does, in IEEE double, left to right, every
 * operation rounded once (the order of RenderDepth):
 *
 *   d   = (double)raw * scale * 16.0 * 12.0
 *   z   = focal_px * baseline_mm / d / 1000.0          (raw == 0 -> +inf)
 *   a   = fabs(z * alpha)
 *   idx = isnan(a) ? 0 : (rint(a) >= 255 ? 255 : (int)rint(a))          (ties to even)
 *
 * A field of scale, focal_px, baseline_mm, alpha that is 0 takes the reference's value (0.00000260443857769133,
 * 527.1931762695312, 119.89382172, 9); all of sn_render_params zero is the reference's render node.
 *
 * Tables (sn_render_tables, pure host): rgb[257][3] and ycc[257][3], entry 256 = "no measurement".
 *   colour map entry i (0..255) as (B, G, R): SN_CMAP_JET = round(255 * clip(1.5 - |4 * i/255 - {1, 2, 3}|, 0, 1)), exactly
 *     JetLutBGR() / render.jet_lut(); SN_CMAP_GREY = (i, i, i).
 *   rgb[i] = the three canvas bytes of index i, in the canvas's R, G, B positions: with true_colours == 0 (the reference's
 *     published picture) the map's (B, G, R) stored as if they were (R, G, B), so rgb[0..255] is the JET table as it stands;
 *     with true_colours != 0 the map's (R, G, B).  rgb[256] is black; it is used for raw == 0 when invalid_black != 0
 *     (the post-processing masks say "no measurement" with raw == 0); otherwise raw == 0 takes idx = 255 as the formula gives.
 *   ycc[i] from the canvas (R, G, B) = rgb[i], JFIF full-range BT.601 in libjpeg's fixed point (>> arithmetic, no clamp needed):
 *     Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
 *     Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
 *     Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
 *
 * Canvas.  layout SN_RENDER_STACK: the left eye on top, the colour map below, Hc = 2H; SN_RENDER_DEPTH: the colour map only,
 *   Hc = H, left_nv12 may be NULL.  The left eye: frame k at left_nv12 + k * left_pitch * (H + ceil(H/2)), H luma rows of
 *   left_pitch bytes and the chroma rows behind them — sn_pointcloud_from_raw's rule: W for a plain left image, 2W for the left
 *   half of a side-by-side frame in place, any even value >= W.
 *   format SN_RENDER_RGB8: frame k at out + k * out_frame, Hc rows of out_pitch >= 3W bytes, pixel = R, G, B.  The left eye is
 *     converted with the integer formula sn_pointcloud_from_raw documents; the colour half is rgb[idx].  In reference mode the
 *     colour half equals RenderDepth's color_bgr and the whole equals StackJoint, byte for byte.  Any W and H.
 *   format SN_RENDER_NV12: Hc luma rows of out_pitch >= W bytes, then Hc/2 chroma rows, as sn_jpeg_encode_nv12 reads them.
 *     The left eye's luma and chroma rows are copied as they are.  Colour half: Y = ycc[idx][0] per pixel; per 2x2 block
 *     Cb = (sum of the four pixels' ycc[.][1] + 2) >> 2, Cr likewise.  W and H must be even.
 *   Bytes between W (3W) and out_pitch are not written; out may be at any address.
 *
 * sn_render_tables: the two tables for p's colormap and true_colours; rgb and ycc may each be NULL.  SN_ERR_ARG: p NULL or an
 *   unknown colour map.
 * sn_render: n maps (1 <= n <= max_batch) raw [n][H][W] -> n canvases.  One kernel launch per call.
 * sn_render_jpeg: exactly the bytes and sizes of sn_jpeg_encode_nv12(w = W, h = Hc, pitch = W, jp) on the SN_RENDER_NV12
 *   canvas of sn_render at pitch W: stream k at out + k * out_stride, its length in sizes[k]; a stream that does not fit gives
 *   sizes[k] = 0 and nothing of it is stored, the other frames are unaffected and the call returns SN_OK.  The canvas lives
 *   in the stage's scratch (eight frames of it) and never crosses to the host.
 * SN_ERR_ARG (sn_last_error(h) says why; nothing is launched or written): n out of range, a required pointer NULL (left_nv12
 *   with SN_RENDER_STACK), an unknown layout, format or colour map, scale, focal_px or baseline_mm negative or not finite, alpha
 *   not finite, left_pitch odd or < W, out_pitch too small, out_frame smaller than a canvas ((rows - 1) * out_pitch + the
 *   bytes of a row), odd W or H with SN_RENDER_NV12 or sn_render_jpeg (and what sn_jpeg_encode_nv12 refuses for W x Hc), out
 *   overlapping raw, left_nv12 or sizes, a bad mem.  SN_ERR_NOMEM: the scratch or the staging could not be allocated.
 * mem / stream as sn_filter_raw: a lane of the handle's with a stream, an event and grow-only scratch of its own (never the
 *   inference stream), freed by sn_destroy; the call returns after completion when mem is SN_MEM_HOST or stream is NULL; device
 *   buffers + a caller stream only enqueue.  May run beside sn_submit / sn_wait and beside the other stages; calls are
 *   serialised by the lane's mutex.  Not covered: the asynchronous sn_submit* slots, colour maps other than the two, a
 *   horizontal stack. */
#define SN_RENDER_STACK 0
#define SN_RENDER_DEPTH 1
#define SN_RENDER_RGB8  0
#define SN_RENDER_NV12  1
#define SN_CMAP_JET     0
#define SN_CMAP_GREY    1
typedef struct sn_render_params {
  double scale, focal_px, baseline_mm, alpha;   /* 0 = the reference's 0.00000260443857769133 / 527.1931762695312 / 119.89382172 / 9 */
  int layout, colormap, true_colours, invalid_black;
} sn_render_params;                             /* all zero = the reference's render node */
int  sn_render_tables(const sn_render_params *p, uint8_t *rgb /*257*3*/, uint8_t *ycc /*257*3*/);   /* pure host */
int  sn_render(sn_handle *h, int n, const int32_t *raw, const uint8_t *left_nv12, int left_pitch, const sn_render_params *p,
               int format, uint8_t *out, int out_pitch, size_t out_frame, int mem, void *stream);
int  sn_render_jpeg(sn_handle *h, int n, const int32_t *raw, const uint8_t *left_nv12, int left_pitch, const sn_render_params *p,
                    const sn_jpeg_params *jp, uint8_t *out, size_t out_stride, uint32_t *sizes, int mem, void *stream);

/* ---- bird's-eye obstacle grid and laser scan from the int32 map (csrc/sn_obstacles.hpp; hobot_stereonet_amd/obstacles.py is
 * the numpy twin, byte for byte) ------------------------------------------------------------------------------------------
 * What a robot needs of the point cloud: where it cannot drive.  A nav_msgs/OccupancyGrid and a sensor_msgs/LaserScan per map,
 * reduced on the device: the call reads the 4 bytes a pixel sn_pointcloud_from_raw reads and writes a few thousand numbers.
 *
 * Points.  The samples are sn_pointcloud_from_raw's: (u, v) = (j*step, i*step) of map k; Z, X, Y and valid exactly as there
 *   (the same device functions), cam's z_min_m / z_max_m / step honoured.  The base frame (x forward, y left, z up) in fp32,
 *   left to right, every operation rounded (no FMA), m = base_from_cam:
 *     xb = ((m0*X + m1*Y) + m2*Z) + m3,   yb likewise from m4..m7,   zb likewise from m8..m11
 *   Class from zb: ground z_floor_m <= zb <= z_lo_m; obstacle z_lo_m < zb <= z_hi_m; anything else (overhead, below the floor,
 *   NaN) counts nowhere.
 * Grid.  qx = floorf((xb - x_min_m) / cell_m), qy likewise from yb and y_min_m; the point is in the grid when
 *   qx >= 0 && qx < (float)gw && qy >= 0 && qy < (float)gh (tested in float before the conversion to int); cell = qy*gw + qx.
 *   hits      [n][gh][gw][2] = {obstacle points, ground points} of the cell
 *   height_mm [n][gh][gw]    = the maximum over the cell's obstacle points of (int)floorf(zb * 1000.f) (saturated to int32),
 *                              INT32_MIN without one
 *   occ       [n][gh][gw]    = 100 when obstacle hits >= min_obstacle_hits, else 0 when ground hits >= min_ground_hits, else -1
 *   stats     [n][4]         = {obstacle points in the grid, ground points in the grid, occupied cells, free cells}
 * Scan.  sn_obstacle_beam_edges: edges[i] = (float)tan((double)angle_min_rad + (double)i * (double)angle_increment_rad),
 *   i = 0..beams; SN_ERR_ARG unless 1 <= beams <= 4096, every angle lies inside (-pi/2, pi/2) and the edges increase strictly.
 *   An obstacle-class point contributes, whether or not the grid holds it, when xb > 0, t = yb / xb has
 *   edges[0] <= t < edges[beams], and r = sqrtf(xb*xb + yb*yb) (two rounded products, one rounded sum) has
 *   range_min_m <= r <= range_max_m.  Its beam is the number of edges <= t, minus 1 (a binary search on the table).
 *   ranges [n][beams] = the minimum r per beam, +inf (bits 0x7f800000) without a return.
 * Every accumulator is an integer (a positive float orders as its bits), so the outputs do not depend on the order in which
 * the points arrive.
 *
 * Every output is nullable; a call needs occ, hits, height_mm or ranges.  The grid outputs (occ, hits, height_mm, stats)
 * require gw, gh > 0, ranges requires beams > 0.  SN_ERR_ARG (sn_last_error(h) says why; nothing is launched or written):
 * n outside 1..max_batch, raw / cam / p NULL, a camera sn_pointcloud_from_raw would refuse, a float of p that is not finite,
 * cell_m <= 0, gw or gh negative or > 4096 or only one of them 0, beams negative or > 4096, z_floor_m > z_lo_m or
 * z_lo_m > z_hi_m, a negative hit threshold, range_min_m < 0 or range_max_m < range_min_m, a sector sn_obstacle_beam_edges
 * refuses (beams > 0), overlapping buffers, a bad mem.  Whether R is a rotation is not checked.
 * mem / stream / blocking and SN_ERR_NOMEM as sn_pointcloud_from_raw: a lane of the handle's with a stream, an event and
 * grow-only buffers of its own, freed by sn_destroy; may run beside sn_submit / sn_wait and beside the other stages.
 * Not covered: the asynchronous sn_submit* slots, beams beyond +-90 degrees, ray clearing of the cells in front of an obstacle,
 * negative obstacles (below z_floor_m), hit thresholds that fall with range. */
typedef struct sn_obstacle_params {
  float base_from_cam[12];          /* row-major 3x4 [R|t], metres: p_base = R p_cam + t.  Camera frame as the point cloud's
                                       (X right, Y down, Z forward); base frame x forward, y left, z up.  All twelve zero =
                                       the level forward mount R = [[0,0,1],[-1,0,0],[0,-1,0]], t = 0 */
  float x_min_m, y_min_m, cell_m;   /* cell (ix, iy) covers [x_min + ix*cell, +cell) x [y_min + iy*cell, +cell) */
  int   gw, gh;                     /* cells along x and y; data index iy*gw + ix (nav_msgs/OccupancyGrid); 0,0 = no grid */
  float z_floor_m, z_lo_m, z_hi_m;  /* ground: z_floor <= zb <= z_lo; obstacle: z_lo < zb <= z_hi; else ignored */
  int   min_obstacle_hits, min_ground_hits;
  int   beams;                      /* 0 = no scan */
  float angle_min_rad, angle_increment_rad, range_min_m, range_max_m;
} sn_obstacle_params;
int sn_obstacle_beam_edges(const sn_obstacle_params *p, float *edges /* beams + 1 */);      /* pure host, no device */
int sn_obstacles_from_raw(sn_handle *h, int n, const int32_t *raw, const sn_camera *cam, const sn_obstacle_params *p,
                          int8_t *occ, uint32_t *hits, int32_t *height_mm, float *ranges, uint32_t *stats,
                          int mem, void *stream);

/* sn_obstacles_from_raw with one mount per map: map k's base_from_cam is the twelve floats at mounts + k * mount_stride
 * (mount_stride >= 12, in floats; host or device memory per `mem`, like every other buffer of the call), used as they are (no
 * all-zero rule), and p->base_from_cam is ignored (it need not be finite).  With &ground[0].base_from_cam[0] and
 * sizeof(sn_ground) / 4 the mounts of sn_ground_from_raw are read where that call left them: on one stream, fit -> grid needs no
 * host round trip.  Everything else, the arithmetic included, is sn_obstacles_from_raw's; a mount that is not finite classifies
 * nothing (NaN counts nowhere).  SN_ERR_ARG also for mounts NULL or misaligned (4 bytes), mount_stride < 12, and mounts that
 * overlap an output. */
int sn_obstacles_from_raw_mounts(sn_handle *h, int n, const int32_t *raw, const sn_camera *cam, const sn_obstacle_params *p,
                                 const float *mounts, int mount_stride, int8_t *occ, uint32_t *hits, int32_t *height_mm,
                                 float *ranges, uint32_t *stats, int mem, void *stream);

/* ---- the ground plane of the int32 map, and the mount it implies (csrc/sn_ground.hpp; hobot_stereonet_amd/ground.py is the
 * numpy twin, byte for byte) --------------------------------------------------------------------------------------------------
 * sn_obstacles_from_raw classifies by height in a base frame that the caller measured once.  This stage measures it per frame
 * from what nearly every map shows: the floor.  For a rectified pinhole pair a plane in space is a plane in (u, v, raw),
 * raw = a*u + b*v + c, so every decision below is taken on integers and the outputs do not depend on the order of arrival.
 *
 * Samples.  The region of interest is roi_x, roi_y, roi_w, roi_h in pixels (all four 0: the lower half at full width, y = H/2,
 *   h = H - H/2).  Its samples are the pixels (u, v) = (j*step, i*step), step = cam->step, with roi_x <= u < roi_x + roi_w and
 *   roi_y <= v < roi_y + roi_h: Ws columns from j0 = ceil(roi_x/step), Hs rows from i0 = ceil(roi_y/step), Ns = Ws*Hs, sample
 *   index s = si*Ws + sj.  (u0, v0) = (roi_x + roi_w/2, roi_y + roi_h/2) (integer division) is the centre the plane's c refers
 *   to.  A sample is usable when 0 < r <= 2^24 (8 388 px of disparity).  cam's z_min_m / z_max_m are not used.
 *   Bounds, W, H <= 8192: |du|, |dv| <= 8191 < 2^13 and |dr| < 2^24, so |C| <= 2 * 2^26 = 2^27 and r <= 2^24 fit in 32 bits,
 *   |A|, |B| <= 2^38, |D| and every residual A*u + B*v + C*r - D stay below 2^54, tol_raw*C <= 2^51; in Q16, |aq|, |bq| <= 2^34
 *   and |cq| <= 2^41 (enforced), so aq*du + bq*dv + cq < 2^49 and r*65536 <= 2^40; the moments are taken of du = u - u0,
 *   dv = v - v0 (|du|, |dv| <= 4097) over Ns <= 2^26 samples, the largest, sum du*r, below 2^26 * 4097 * 2^24 < 2^63.
 * Hypotheses.  K = hypotheses, 1..1024.  mix(seed, i): x = seed + i*0x9E3779B9; x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15;
 *   x *= 0x846CA68B; x ^= x >> 16 (all uint32).  Hypothesis i takes the samples s_j = mix(seed, 3*i + j) % Ns, j = 0, 1, 2, the
 *   same for every map of the call.  With d1 = P1 - P0, d2 = P2 - P0 in (u, v, r): A = d1v*d2r - d1r*d2v, B = d1r*d2u - d1u*d2r,
 *   C = d1u*d2v - d1v*d2u; all three negated when C < 0; D = A*u_0 + B*v_0 + C*r_0.  The hypothesis is dead when a sample is not
 *   usable, when C < max(min_area, 1), or when it lies outside the gate:
 *     gate[0]*C <= -A*65536 <= gate[1]*C,  gate[2]*C <= -B*65536 <= gate[3]*C,
 *     gate[4]*C <= (D - A*u0 - B*v0)*65536 <= gate[5]*C     (this last pair needs 70 bits: 128-bit integers)
 * Gate.  sn_ground_gate (pure host, no device) turns the prior mount m = base_from_cam (all twelve zero: the level forward
 *   mount), max_tilt_rad and the two heights into Q16 bounds on a = -A/C, b = -B/C and c, the plane's value at (u0, v0).  In
 *   double, S = (double)(float)((double)out_scale * 192.0), Bm = (double)baseline_mm / 1000.0, x0 = (m0, m1, m2),
 *   y0 = (m4, m5, m6), n0 = -(m8, m9, m10); for alpha and beta in {0, -max_tilt_rad, +max_tilt_rad} (alpha outer) and
 *   h in {height_min_m, height_max_m} (innermost):
 *     n = cos(beta)*(cos(alpha)*n0 + sin(alpha)*y0) + sin(beta)*x0,  g = Bm / (h*S),
 *     a = g*n_x,  b = g*n_y*fx/fy,  cp = g*n_z*fx,  c = (cp + a*(u0 - cx)) + b*(v0 - cy)
 *   gate[0], gate[1] = floor(min a*65536), ceil(max a*65536) over the eighteen planes, gate[2..3] likewise from b, gate[4..5]
 *   from c; the first four clamped to +-2^34, the last two to +-2^41.  A wall is often the largest plane in view: for a level
 *   prior the gate keeps b well above 0, which a fronto-parallel wall (a = b = 0) is not.  The device never calls a
 *   transcendental function; a twin is fed the library's gate, as it is fed the library's beam table.
 * Score.  tol_raw = (int64)floorf(tol_px / S) with S = (float)((double)out_scale * 192.0), sn_temporal's rule; it must not
 *   exceed 2^24.  A usable sample is an inlier of a live hypothesis when |A*u + B*v + C*r - D| <= tol_raw*C.  The winner is the
 *   live hypothesis with the highest count, ties to the lowest index.  Its plane in Q16, q(x) = (int64)floor(x*65536 + 0.5) with
 *   x a correctly rounded double quotient: aq = q(-A / C), bq = q(-B / C), cq = q((D - A*u0 - B*v0) / C).
 * Refit, `refits` (0..4) times.  A usable sample is an inlier of a Q16 plane when
 *     |r*65536 - (aq*(u - u0) + bq*(v - v0) + cq)| <= tol_raw*65536.
 *   Over the inliers, with du = u - u0, dv = v - v0, nine int64 moments: N, Su, Sv, Sr, Suu, Suv, Svv, Sur, Svr.  Each is
 *   converted to double (round to nearest), then, in double, every operation rounded, no FMA:
 *     mu = Su/N, mv = Sv/N, mr = Sr/N,
 *     suu = Suu - Su*mu, suv = Suv - Su*mv, svv = Svv - Sv*mv, sur = Sur - Su*mr, svr = Svr - Sv*mr,
 *     det = suu*svv - suv*suv,  a = (sur*svv - svr*suv)/det,  b = (svr*suu - sur*suv)/det,  c = (mr - a*mu) - b*mv
 *   and (aq, bq, cq) = (q(a), q(b), q(c)).  The system is singular when N < 3, when det > 0 does not hold, or when |a*65536| or
 *   |b*65536| exceeds 2^34 or |c*65536| exceeds 2^41 (NaN included): the previous plane stays, no further refit is made, and
 *   SN_GROUND_SINGULAR is set (a note, not a failure).  `inliers` is the count under the final plane.
 * Result.  SN_GROUND_NO_HYPOTHESIS: no hypothesis is live (winner = -1, plane_q16 = 0, inliers = 0).  Else
 *   SN_GROUND_FEW_INLIERS: inliers < min_inliers.  Else SN_GROUND_GATED: the final plane is outside the gate (the six bounds
 *   on aq, bq, cq as integers) or the geometry below fails.  Else SN_GROUND_FOUND.  Without SN_GROUND_FOUND, plane_cam is
 *   (-m8, -m9, -m10, m11) and base_from_cam the prior mount (the level mount written out where the prior is all zero), so what
 *   follows stays defined.
 * Geometry, in double, every operation rounded, no FMA, only + - * / and sqrt; then rounded to float:
 *     a = aq/65536, b = bq/65536, c = cq/65536,  cp = (c + a*(cx - u0)) + b*(cy - v0),
 *     w = (a, (b*fy)/fx, cp/fx),  len = sqrt((w0*w0 + w1*w1) + w2*w2)   (0 or not finite: gated),
 *     height = (baseline_mm/1000) / (S*len),  the downward normal n = w/len,  plane_cam = (n, height)
 *   The mount keeps the prior's heading and horizontal offset and replaces tilt and height: z = -n,
 *   d = (x0_0*z_0 + x0_1*z_1) + x0_2*z_2, x' = x0 - d*z, |x'| = sqrt((x'_0^2 + x'_1^2) + x'_2^2) (below 1e-3: gated),
 *   x = x'/|x'|, y = z cross x = (z1*x2 - z2*x1, z2*x0 - z0*x2, z0*x1 - z1*x0), base_from_cam = rows (x, m3), (y, m7),
 *   (z, height).  A level camera 0.5 m above a level floor gives back the level mount with t_z = 0.5.
 *   The integer outputs (flags, counts, plane_q16, labels) are exact on every input.  The float outputs are the same bits
 *   as the twin's wherever double division and sqrt are correctly rounded on both sides, which they are on gfx950 and in numpy.
 * Labels (nullable), uint8 [n][H][W], every pixel of the map, not only the region or the step grid: SN_GROUND_LABEL_NONE where
 *   the pixel is not usable; else SN_GROUND_LABEL_NO_PLANE without SN_GROUND_FOUND; else, with
 *   e = r*65536 - (aq*(u - u0) + bq*(v - v0) + cq): GROUND when |e| <= tol_raw*65536, ABOVE when e is larger (nearer than the
 *   floor: something stands there), BELOW when smaller (a hole, a step down).
 *
 * ground (nullable) [n]; one of ground and labels is needed.  SN_ERR_ARG (sn_last_error(h) says why; nothing is launched or
 * written): n outside 1..max_batch, raw / cam / p NULL, a camera sn_pointcloud_from_raw refuses or whose cx, cy are not finite,
 * a float of p that is not finite, hypotheses outside 1..1024, refits outside 0..4, min_area or min_inliers negative, tol_px
 * negative or tol_raw > 2^24, max_tilt_rad outside [0, 1.5], height_min_m <= 0 or height_max_m < height_min_m, a region that
 * leaves the image or holds fewer than three samples, W or H above 8192, ground misaligned (8 bytes), overlapping buffers, a bad
 * mem.  mem / stream / blocking and SN_ERR_NOMEM as sn_obstacles_from_raw: a lane of the handle's with a stream, an event and
 * grow-only buffers of its own, freed by sn_destroy; may run beside sn_submit / sn_wait and beside the other stages.
 * Not covered: the asynchronous sn_submit* slots, smoothing the plane over time, publishing the mount as a transform, more
 * than one plane (a ramp ahead), uneven ground, yaw and the horizontal offset (which a plane cannot give). */
enum { SN_GROUND_FOUND = 1, SN_GROUND_NO_HYPOTHESIS = 2, SN_GROUND_FEW_INLIERS = 4, SN_GROUND_GATED = 8, SN_GROUND_SINGULAR = 16 };
enum { SN_GROUND_LABEL_NONE = 0, SN_GROUND_LABEL_GROUND = 1, SN_GROUND_LABEL_ABOVE = 2, SN_GROUND_LABEL_BELOW = 3,
       SN_GROUND_LABEL_NO_PLANE = 4 };
typedef struct sn_ground_params {
  float base_from_cam[12];          /* the prior mount, as sn_obstacle_params' (all twelve zero: the level forward mount) */
  int   roi_x, roi_y, roi_w, roi_h; /* pixels; all four 0: the lower half of the image at full width */
  int   hypotheses;                 /* K, 1..1024 */
  uint32_t seed;
  int   min_area;                   /* a hypothesis needs C (twice its triangle's area, in pixels^2) >= max(min_area, 1) */
  int   min_inliers;
  int   refits;                     /* 0..4 */
  float tol_px;                     /* inlier band, pixels of disparity */
  float max_tilt_rad;               /* the gate: tilt about the prior's x and y axes */
  float height_min_m, height_max_m; /* the gate: camera height above the plane */
} sn_ground_params;
typedef struct sn_ground {
  uint32_t flags;                   /* SN_GROUND_* */
  uint32_t usable;                  /* usable samples of the region */
  uint32_t inliers;                 /* under the final plane */
  int32_t  winner;                  /* index of the winning hypothesis, -1 without one */
  uint32_t survivors;               /* live hypotheses */
  uint32_t reserved;                /* 0 */
  int64_t  plane_q16[3];            /* aq, bq, cq: raw*65536 = aq*(u - u0) + bq*(v - v0) + cq */
  float    plane_cam[4];            /* the downward unit normal in the camera frame, and the height in metres */
  float    base_from_cam[12];       /* the mount: sn_obstacles_from_raw_mounts reads it here */
} sn_ground;
int sn_ground_gate(const sn_camera *cam, const sn_ground_params *p, int W, int H, int64_t gate[6]);      /* pure host, no device */
int sn_ground_from_raw(sn_handle *h, int n, const int32_t *raw, const sn_camera *cam, const sn_ground_params *p,
                       sn_ground *ground, uint8_t *labels, int mem, void *stream);

/* ---- rolling log-odds costmap with ray clearing, one map per STREAM (csrc/sn_costmap.hpp; hobot_stereonet_amd/costmap.py is
 * the numpy twin, byte for byte) --------------------------------------------------------------------------------------------------
 * sn_obstacles_from_raw answers for one frame: a cell is free only where enough ground points landed in it, and the answer is
 * forgotten at the next frame.  sn_costmap accumulates the grid and the scan over time as log-odds in a window that travels
 * with the robot (costmap_2d's rolling window with an inverse sensor model), and clears the cells a beam crossed in front of
 * its return.  It takes occ and ranges where the obstacle stage left them, and the robot's planar pose per frame.  Everything
 * below the pose quantisation is integer apart from two single rounded double multiplies, so no tolerance appears anywhere.
 *
 * `op` is the block the caller gives the obstacle stage: cell_m, gw, gh, x_min_m, y_min_m describe the base-frame grid that
 *   occ is in, beams, the angles and sn_obstacle_beam_edges describe ranges; the base frame is that stage's (x forward, y left).
 *   The map's cells are cell_m wide as well.
 * Units.  A "sub" is 1/256 of a cell.  Host quantities, in double, computed once (or per pose) and passed to the kernel as
 *   integers, the one double k256 apart:
 *     k256 = 256.0 / (double)cell_m,   gx0 = llrint((double)x_min_m / (double)cell_m * 256.0), gy0 likewise from y_min_m
 *       (beyond +-2^40 taken as +-2^40: no cell reaches that far),
 *     margin = llrint((double)clear_margin_m * k256), rmin and cmax likewise from clear_min_m and clear_max_m (above 2^31
 *       taken as 2^31: r2 below stays under 2^42),
 *   sn_costmap_pose_q (pure host, no device): q = {tx, ty, cq, sq, ox, oy} with tx = llrint(x * k256), ty likewise,
 *     cq = llrint(cos(yaw) * 2^30), sq = llrint(sin(yaw) * 2^30), ox = (tx >> 8) - mw/2, oy = (ty >> 8) - mh/2 (>> arithmetic,
 *     / integer division).  SN_ERR_ARG for a pose that is not finite or has |x| * k256 or |y| * k256 above 2^30.  Two
 *     implementations of a double cos may differ by an ulp: a twin is fed the library's q, as it is fed the library's beam table.
 * State per stream: int16 L[mh][mw], -32768 = unknown.  The map is a torus: world cell (cx, cy) lives in slot
 *   (cx mod mw, cy mod mh) (floor modulo); after a frame with origin (ox, oy), slot (i, j) holds the world cell
 *   cx = ox + ((i - ox) mod mw), cy = oy + ((j - oy) mod mh).  A fresh or reset stream is all unknown and has no previous origin.
 * One frame of a stream, per slot, in this order:
 *   1. Scroll.  Where the stream has a previous origin and the slot's world cell under it differs from the one under the new
 *      origin, L = unknown (a jump of more than a window clears everything; nothing is copied).
 *   2. The cell's centre in the base frame, in int64, >> arithmetic:
 *        dx = cx*256 + 128 - tx, dy = cy*256 + 128 - ty,
 *        bx = (cq*dx + sq*dy + 2^29) >> 30,   by = (-sq*dx + cq*dy + 2^29) >> 30
 *   3. Grid observation.  qx = (bx - gx0) >> 8, qy = (by - gy0) >> 8; o = occ[qy][qx] inside 0..gw-1 x 0..gh-1, else -1.
 *   4. Ray, only when bx > 0.  With E[i] = (double)edges[i], the cell is in the sector when E[0]*(double)bx <= (double)by and
 *      not E[beams]*(double)bx <= (double)by; its beam b is (the number of i with E[i]*(double)bx <= (double)by) - 1 (each
 *      comparison one rounded double product, monotone in i: a binary search).
 *        Rb = ranges[b] finite and > 0 ? min((int64)floor((double)ranges[b] * k256), 2^31 - 1) : -1   (no return: clears nothing)
 *        C = Rb - margin,  r2 = bx*bx + by*by,
 *        ray = Rb >= 0 && C > 0 && r2 < C*C && r2 >= rmin*rmin && (cmax == 0 || r2 <= cmax*cmax)
 *   5. Log-odds, with L0 = (L unknown ? 0 : L):  o == 100: L = min(L0 + l_hit, l_max), a hit;  otherwise, o == 0 || ray:
 *      L = max(L0 - l_miss, l_min), cleared;  otherwise L stays.
 * Outputs, unrolled in nav_msgs/OccupancyGrid order: element [cy - oy][cx - ox] of map k.
 *   grid    int8  [n][mh][mw] = -1 for unknown, else ((L - l_min)*100 + (l_max - l_min)/2) / (l_max - l_min)
 *   logodds int16 [n][mh][mw] = L
 *   stats   [n][4] = {known cells, cells with L > 0, hits this frame, cleared this frame}
 *   At least one of the three is required.  pose_q_out (nullable, HOST, [n][6]) receives the q of every map.
 * sn_costmap_create: `streams` independent maps (1 <= streams <= max_batch) on handle h, all fresh; the state
 *   (2 * mh * mw * streams bytes), the beam table, a stream, an event and the host-mode staging are the object's own.
 *   h == NULL makes a host-only object (any streams >= 1) that serves sn_costmap_pose_q alone and touches no device;
 *   sn_costmap_push on it is SN_ERR_ARG.
 *   SN_ERR_ARG: a NULL pointer, streams out of range, mw or mh outside 1..4096, l_hit or l_miss outside 1..32767, not
 *   -32767 <= l_min < 0 < l_max <= 32767, a negative clear_*, a float of p or cell_m, x_min_m, y_min_m that is not finite,
 *   cell_m <= 0, gw or gh negative or > 4096 or only one of them 0, beams negative or > 4096, a sector sn_obstacle_beam_edges
 *   refuses (beams > 0), neither a grid nor a scan.  While a costmap is alive sn_destroy(h) is REFUSED with SN_ERR_BUSY, as for
 *   sn_temporal.
 * sn_costmap_reset: stream `stream` (-1: all) is fresh again.  A host-side flag that takes effect at the next push.
 *   SN_ERR_ARG: an id outside -1..streams-1.
 * sn_costmap_push: n maps (1 <= n <= max_batch); map k is the next frame of stream stream_of[k] (a host array; NULL: all of
 *   stream 0, one clip) at pose poses[k] = {x, y, yaw} (metres, radians; always HOST memory).  Maps with the same id are
 *   consecutive frames in the order of k, and a push of n maps equals n single pushes in that order, bit for bit.
 *   occ [n][gh][gw] and ranges [n][beams] as sn_obstacles_from_raw wrote them.  Either may be absent (occ NULL or gw == 0;
 *   ranges NULL or beams == 0), but not both.
 *   SN_ERR_ARG (sn_last_error(h) names the call; nothing is launched or written and no state changes): n out of range, poses
 *     NULL, a pose sn_costmap_pose_q refuses, neither occ nor ranges usable, no output, an id outside 0..streams-1, logodds
 *     misaligned (2 bytes), stats or ranges misaligned (4 bytes), overlapping buffers, a bad mem.
 *   mem / stream as sn_temporal_push: a NULL stream is the costmap's own stream (never the inference stream); the call
 *   returns after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller stream only enqueue, so
 *   ground -> obstacles -> costmap run on one stream without a host round trip.  May run beside sn_submit / sn_wait and the
 *   other stages; calls are serialised by the object's mutex.  One kernel launch per 64 maps of a call.
 * Not covered: the asynchronous sn_submit* slots, decay of unobserved cells, 3-D voxels, clearing along beams without a
 * return, poses with roll or pitch.  (Inflation by the robot's radius is sn_inflate_grid below.) */
typedef struct sn_costmap_params {
  int   mw, mh;                      /* window in cells, 1..4096 each */
  int   l_hit, l_miss;               /* 1..32767 */
  int   l_min, l_max;                /* -32767 <= l_min < 0 < l_max <= 32767 */
  float clear_margin_m;              /* >= 0: a ray clears only up to this far in front of its return */
  float clear_min_m, clear_max_m;    /* >= 0; clear_max_m == 0: no cap */
} sn_costmap_params;
typedef struct sn_costmap sn_costmap;
int  sn_costmap_create(sn_handle *h, int streams, const sn_obstacle_params *op, const sn_costmap_params *p, sn_costmap **out);
int  sn_costmap_reset(sn_costmap *c, int stream);
void sn_costmap_destroy(sn_costmap *c);
int  sn_costmap_pose_q(const sn_costmap *c, const double pose[3] /* x, y, yaw */, int32_t q[6]);   /* pure host */
int  sn_costmap_push(sn_costmap *c, int n, const int *stream_of, const double *poses /* host [n][3] */,
                     const int8_t *occ /* [n][gh][gw] */, const float *ranges /* [n][beams] */,
                     int8_t *grid /* [n][mh][mw] */, int16_t *logodds /* [n][mh][mw] */, uint32_t *stats /* [n][4] */,
                     int32_t *pose_q_out /* host [n][6], nullable */, int mem, void *stream);

/* ---- rolling elevation map and step-height traversability, one map per STREAM (csrc/sn_elevation.hpp;
 * hobot_stereonet_amd/elevation.py is the numpy twin, byte for byte) ------------------------------------------------------------
 * sn_obstacles_from_raw assumes a flat floor at z = 0 of the base frame: a ramp reads as a wall, a drop as nothing, a kerb
 * below z_lo_m as free.  sn_elevation keeps a 2.5-D map instead (elevation mapping, grid_map): per cell of a window that travels
 * with the robot the highest and the lowest height seen, fused over time, and judges a cell by the height differences to its
 * neighbours, not by a fixed band.  The verdict is an OccupancyGrid payload, so sn_inflate_grid -> sn_navfn -> sn_rollout take
 * it as they take the costmap's grid.  Everything below the pose quantisation is integer or a single rounded fp32 operation
 * in a stated order, so no tolerance appears anywhere.
 *
 * Units.  A "sub" is 1/256 of a cell; heights are millimetres.  Host quantities, computed once:
 *     k256 = 256.0 / (double)cell_m,  k256f = (float)k256,
 *     zmin_mm = (int)floorf(z_min_m * 1000.f),  zmax_mm = (int)floorf(z_max_m * 1000.f)     (one rounded fp32 product each)
 *   sn_elevation_pose_q (pure host, no device) is sn_costmap_pose_q's rule with this object's cell_m, mw, mh:
 *     q = {tx, ty, cq, sq, ox, oy}, tx = llrint(x * k256), ty likewise, cq = llrint(cos(yaw) * 2^30), sq = llrint(sin(yaw) * 2^30),
 *     ox = (tx >> 8) - mw/2, oy = (ty >> 8) - mh/2; SN_ERR_ARG for a pose that is not finite or has |x| * k256 or |y| * k256
 *     above 2^30.  A twin is fed the library's q.
 * State per stream: two int16 planes hi[mh][mw] and lo[mh][mw] in millimetres, -32768 = unknown (a cell is known where hi is
 *   not unknown; lo is unknown exactly where hi is).  The planes live on the costmap's torus: world cell (cx, cy) in slot
 *   (cx mod mw, cy mod mh) (floor modulo); after a frame with origin (ox, oy), slot (i, j) holds the world cell
 *   cx = ox + ((i - ox) mod mw), cy = oy + ((j - oy) mod mh).  A fresh or reset stream is all unknown and has no previous origin.
 * One frame of a stream at pose q, in this order:
 *   1. Scroll.  Where the stream has a previous origin and a slot's world cell under it differs from the one under the new
 *      origin, hi = lo = unknown (a jump of more than a window clears everything; nothing is copied).
 *   2. Frame accumulators, per cell of the frame's window: cnt = 0, fmax = INT32_MIN, fmin = INT32_MAX, then every sample:
 *      The samples are sn_pointcloud_from_raw's: (u, v) = (j*step, i*step) of the map; Z, X, Y and valid exactly as there,
 *      cam's z_min_m / z_max_m / step honoured.  xb, yb, zb are sn_obstacles_from_raw's (the same device functions: fp32, left
 *      to right, every operation rounded, no FMA), with m = base_from_cam (all twelve zero: the level forward mount), or, where
 *      `mounts` is not NULL, map k's twelve floats at mounts + k * mount_stride used as they are (the semantics of
 *      sn_obstacles_from_raw_mounts; base_from_cam is then ignored and need not be finite).  A sample counts nowhere unless it
 *      passes every test of this list, in this order:
 *        valid, and zb is not NaN;
 *        zmm = (int)floorf(zb * 1000.f), saturated to int32, has zmin_mm <= zmm <= zmax_mm;
 *        sqrtf(xb*xb + yb*yb) <= range_max_m (two rounded products, one rounded sum: the obstacle stage's r; NaN fails);
 *        sx = floorf(xb * k256f), sy = floorf(yb * k256f) (one rounded product each) have |sx| < 2^30 and |sy| < 2^30,
 *          compared in float;
 *        in int64, >> arithmetic:  wx = tx + ((cq*sx - sq*sy + 2^29) >> 30),   wy = ty + ((sq*sx + cq*sy + 2^29) >> 30);
 *          the world cell (wx >> 8, wy >> 8) lies in the window: ox <= (wx >> 8) < ox + mw and oy <= (wy >> 8) < oy + mh.
 *      For the cell: cnt += 1, fmax = max(fmax, zmm), fmin = min(fmin, zmm).  Integer accumulators only: the order of arrival
 *      cannot matter.  (|cq|, |sq| <= 2^30 and |sx|, |sy| < 2^30, so every product stays below 2^60.)
 *   3. Fuse, per slot whose cell has cnt >= min_points, in int32 with an arithmetic shift:
 *        unknown:    hi = clamp(fmax), lo = clamp(fmin);
 *        otherwise:  hi = clamp(hi + (((fmax - hi) * alpha + 128) >> 8)),  lo = clamp(lo + (((fmin - lo) * alpha + 128) >> 8)),
 *      clamp(v) = min(max(v, -32767), 32767).  alpha = 256 replaces the old value.  A slot with fewer points keeps its state.
 *   4. Verdict, on the window's planes after the fuse.  For a known cell c, N = the known cells of its (2*radius + 1)^2
 *      neighbourhood clipped to the window, c included:
 *        rise(c) = max over n in N of max(hi_n - lo_c, hi_c - lo_n)      (>= hi_c - lo_c >= 0, <= 65534)
 *        trav(c) = 100 where rise(c) > max_step_mm, else 0;   unknown cells: trav = -1, rise = 0.
 *      Slopes.  A plane of slope s reads about (2*radius + 1) * cell_m * tan(s) between the far cells of the neighbourhood
 *      (2*radius cells between their centres, plus a cell's own spread between its hi and its lo), so max_step_mm also sets
 *      the steepest drivable ramp: tan(s_max) ~ max_step_mm / (1000 * (2*radius + 1) * cell_m).  With cell_m = 0.1, radius 1
 *      and max_step_mm = 60 that is 11 degrees, and a 6 cm kerb inside one neighbourhood is lethal.  A separate slope or
 *      roughness term is not covered.
 * Outputs, unrolled in nav_msgs/OccupancyGrid order: element [cy - oy][cx - ox] of map k.  Each is nullable; one is required.
 *   trav  int8   [n][mh][mw]
 *   hi    int16  [n][mh][mw],  lo likewise (-32768 = unknown)
 *   rise  uint16 [n][mh][mw]   (saturated to 65535)
 *   stats uint32 [n][4] = {known cells, lethal cells (trav == 100), cells fused this frame (cnt >= min_points), points used
 *                          (the sum of cnt over the window)}
 *   pose_q_out (nullable, HOST, [n][6]) receives the q of every map.
 * sn_elevation_create: `streams` independent maps (1 <= streams <= max_batch) on handle h, all fresh; the state
 *   (4 * mh * mw * streams bytes), a stream, an event, the scratch and the host-mode staging are the object's own.
 *   h == NULL makes a host-only object (any streams >= 1) that serves sn_elevation_pose_q alone and touches no device;
 *   sn_elevation_push on it is SN_ERR_ARG.
 *   SN_ERR_ARG: a NULL pointer, streams out of range, mw or mh outside 1..4096, a float that is not finite, cell_m <= 0,
 *   z_min_m or z_max_m outside [-32, 32] or z_min_m > z_max_m, range_max_m <= 0, min_points < 1, alpha outside 1..256,
 *   max_step_mm outside 1..32767, radius outside 1..3, flags != 0.  While an elevation object is alive sn_destroy(h) is REFUSED
 *   with SN_ERR_BUSY, as for sn_costmap.
 * sn_elevation_reset: stream `stream` (-1: all) is fresh again.  A host-side flag that takes effect at the next push.
 *   SN_ERR_ARG: an id outside -1..streams-1.
 * sn_elevation_push: n maps (1 <= n <= max_batch); map k is the next frame of stream stream_of[k] (a host array; NULL: all of
 *   stream 0, one clip) at pose poses[k] = {x, y, yaw} (metres, radians; always HOST memory).  Maps with the same id are
 *   consecutive frames in the order of k, and a push of n maps equals n single pushes in that order, bit for bit.
 *   SN_ERR_ARG (sn_last_error(h) names the call; nothing is launched or written and no state changes): n out of range, raw,
 *     cam or poses NULL, a camera sn_pointcloud_from_raw refuses, a pose sn_elevation_pose_q refuses, no output, an id outside
 *     0..streams-1, raw, stats or mounts misaligned (4 bytes), hi, lo or rise misaligned (2 bytes), mounts with
 *     mount_stride < 12, overlapping buffers (an input with an output, or two outputs), a bad mem.
 *   Scratch, the object's own and grow-only: 12 bytes per cell and frame for the accumulators, and 2 more for each of hi and lo
 *     that the caller does not take (the verdict reads them).  SN_ERR_NOMEM where it cannot be had; nothing is written then.
 *   mem / stream as sn_costmap_push: a NULL stream is the object's own stream (never the inference stream); the call returns
 *   after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller stream only enqueue, so
 *   ground -> elevation -> inflate run on one stream without a host round trip (mounts = &ground[0].base_from_cam[0],
 *   mount_stride = sizeof(sn_ground) / 4).  May run beside sn_submit / sn_wait and the other stages; calls are serialised by
 *   the object's mutex.  Four kernel launches per call of up to 64 maps: clear, scatter, fuse, verdict (two more per further
 *   64 maps).
 * Not covered: the asynchronous sn_submit* slots, a slope or roughness term, several layers (bridges, tables), cells hidden
 * below an edge (they stay unknown), variance-weighted fusion, poses with roll or pitch. */
typedef struct sn_elevation_params {
  int   mw, mh;                      /* window in cells, 1..4096 each */
  float cell_m;                      /* > 0 */
  float base_from_cam[12];           /* the mount, as sn_obstacle_params' (all twelve zero: the level forward mount) */
  float z_min_m, z_max_m;            /* -32 <= z_min_m <= z_max_m <= 32; z_max_m is the robot's clearance: overhangs are ignored */
  float range_max_m;                 /* > 0: stereo depth error grows with Z^2 */
  int   min_points;                  /* >= 1: points a cell needs in a frame to be fused */
  int   alpha;                       /* 1..256: the weight of the new frame in 1/256 */
  int   max_step_mm;                 /* 1..32767 */
  int   radius;                      /* 1..3: the neighbourhood of the verdict, in cells */
  int   flags;                       /* none defined yet: must be 0 */
} sn_elevation_params;
typedef struct sn_elevation sn_elevation;
int  sn_elevation_create(sn_handle *h, int streams, const sn_elevation_params *p, sn_elevation **out);
int  sn_elevation_reset(sn_elevation *e, int stream);
void sn_elevation_destroy(sn_elevation *e);
int  sn_elevation_pose_q(const sn_elevation *e, const double pose[3] /* x, y, yaw */, int32_t q[6]);   /* pure host */
int  sn_elevation_push(sn_elevation *e, int n, const int *stream_of, const double *poses /* host [n][3] */,
                       const int32_t *raw /* [n][H][W] */, const sn_camera *cam, const float *mounts, int mount_stride,
                       int8_t *trav, int16_t *hi, int16_t *lo, uint16_t *rise /* each [n][mh][mw] */, uint32_t *stats /* [n][4] */,
                       int32_t *pose_q_out /* host [n][6], nullable */, int mem, void *stream);

/* ---- inflation of occupancy grids by the robot's radius (csrc/sn_inflate.hpp; hobot_stereonet_amd/inflate.py is the numpy
 * twin, byte for byte) -----------------------------------------------------------------------------------------------------------
 * A planner treats the robot as a point, so every cell is first charged for how close it lies to an obstacle: lethal at the
 * obstacle, "inscribed" within the robot's inner radius, an exponential fall-off out to the inflation radius (the inflation
 * layer of a navigation stack, directly above the rolling window).  sn_inflate_grid does that for n OccupancyGrid payloads as
 * sn_obstacles_from_raw (occ) and sn_costmap_push (grid) write them: -1 unknown, 0..100 known.  The stage is stateless and
 * integer below one host-built table, so no tolerance appears anywhere.  The distance is the EXACT Euclidean distance to the
 * nearest obstacle cell (a bounded distance transform), not the wavefront approximation of costmap_2d, whose cells inherit
 * the obstacle of the neighbour that reached them first.
 *
 * The host table (sn_inflate_table: pure host, no device), in double, in this order of operations:
 *   R = (int)ceil((double)inflation_radius_m / (double)cell_m); R above SN_INFLATE_MAX_R is refused.
 *   T[0] = 254.  For d2 = 1..R*R:  dist = sqrt((double)d2) * (double)cell_m;
 *     dist <= (double)inscribed_radius_m: T[d2] = 253;   dist > (double)inflation_radius_m: T[d2] = 0;   otherwise
 *     T[d2] = (uint8_t)(252.0 * exp(-(double)cost_scaling * (dist - (double)inscribed_radius_m))), truncated.
 *   T does not increase with d2: the library asserts so after building the table and refuses the parameters otherwise.
 *   Two implementations of a double exp may differ by an ulp, so an entry may differ by one between them: a twin is fed the
 *   library's table, as it is fed the beam table and the costmap's q.
 *   *R (nullable) receives R, table (nullable) its R*R + 1 bytes: call it once for R, then with a table of that size.
 *   SN_ERR_ARG: p NULL, cell_m not finite or <= 0, inscribed_radius_m not finite or negative, inflation_radius_m not finite or
 *   below inscribed_radius_m, cost_scaling not finite or negative, R above 64, lethal_min outside 1..100, flags with bits
 *   other than SN_INFLATE_UNKNOWN, a table that increases.
 * Per cell (x, y) of map k, all integer:
 *   cell (x', y') is an obstacle when occ[k][y'][x'] >= lethal_min (the input is read as trinary: unknown, free, obstacle);
 *   d2 = min (x - x')^2 + (y - y')^2 over the obstacles of the same map; there are no obstacles outside the grid;
 *   c  = d2 <= R*R ? T[d2] : 0;
 *   cost: a known cell (occ >= 0) costs c; an unknown cell costs c when (flags & SN_INFLATE_UNKNOWN ? c > 0 : c >= 253)
 *     and 255 otherwise.
 * Outputs, each [n][gh][gw], each nullable, at least one required:
 *   cost  uint8
 *   grid  int8, the usual publisher translation of cost: 0 -> 0, 253 -> 99, 254 -> 100, 255 -> -1, otherwise
 *         1 + 97 * (cost - 1) / 251 (integer division)
 *   dist2 uint16: d2 where d2 <= R*R, else 0xFFFF
 *   stats uint32 [n][5] = {cells at 254, at 253, at 1..252, at 0, at 255}; they sum to gw * gh.
 * sn_inflate_grid: SN_ERR_ARG is decided before anything is launched or written (sn_last_error(h) names the call): a NULL h, p
 *   or occ, n outside 1..max_batch, gw or gh outside 1..4096, any parameter sn_inflate_table refuses, no output, dist2
 *   misaligned (2 bytes), stats misaligned (4 bytes), any output overlapping occ or another output (a cell reads a halo of R
 *   cells around it, so the call cannot work in place), a bad mem.
 *   mem / stream as sn_obstacles_from_raw: the stage has its own lane on the handle; a NULL stream is the lane's own (never the
 *   inference stream); the call returns after completion when mem is SN_MEM_HOST or stream is NULL; device buffers + a caller
 *   stream only enqueue, so obstacles -> costmap -> inflate run on one stream without a host round trip.  May run beside
 *   sn_submit / sn_wait and the other stages; calls are serialised by the lane's mutex.  One kernel launch per call.
 *   The table of the last parameter block stays on the device: a call with the same block uploads nothing, one with
 *   another block uploads its table behind the lane's earlier calls and waits for the upload.
 * Not covered: the asynchronous sn_submit* slots, non-circular footprints, per-cell own costs (a known cell below lethal_min
 * counts as free whatever its value), a cost that depends on heading. */
#define SN_INFLATE_MAX_R   64
#define SN_INFLATE_UNKNOWN 1     /* flags: an unknown cell takes any cost > 0 (otherwise only costs >= 253) */
typedef struct sn_inflate_params {
  float cell_m;               /* > 0, finite: the grid's cell */
  float inscribed_radius_m;   /* >= 0 */
  float inflation_radius_m;   /* >= inscribed_radius_m */
  float cost_scaling;         /* >= 0, finite */
  int   lethal_min;           /* 1..100: a cell with occ >= lethal_min is an obstacle */
  int   flags;                /* SN_INFLATE_UNKNOWN or 0 */
} sn_inflate_params;
int sn_inflate_table(const sn_inflate_params *p, uint8_t *table /* [R*R+1], nullable */, int *R);   /* pure host, no device */
int sn_inflate_grid(sn_handle *h, int n, const int8_t *occ /* [n][gh][gw] */, int gw, int gh, const sn_inflate_params *p,
                    uint8_t *cost, int8_t *grid, uint16_t *dist2 /* each [n][gh][gw] */, uint32_t *stats /* [n][5] */,
                    int mem, void *stream);

/* ---- navigation function and path to a goal over inflated grids (csrc/sn_navfn.hpp; hobot_stereonet_amd/navfn.py is the
 * numpy twin, byte for byte) ---------------------------------------------------------------------------------------------------
 * What every consumer of an inflated grid does next: a cost-to-go field from a goal cell (the navigation function of navfn)
 * and the path that follows it down from the robot's cell.  sn_navfn does that for n cost grids as sn_inflate_grid writes
 * them.  Everything is integer, and the field is the unique fixed point of min-plus relaxation, so any schedule that
 * converges gives the same words: no tolerance appears anywhere.
 *
 * Input.  cost uint8 [n][gh][gw]: 0 free, 1..252 graded, 253 inscribed, 254 lethal, 255 unknown.  goals int32 [n][2] and
 *   starts int32 [n][2] (nullable), each {x, y} in cells, in the same memory kind as the other buffers.
 * Passable cells and their weight.  A cell of 255 is blocked unless flags has SN_NAV_UNKNOWN_OK, and with it is priced as
 *   cost' = unknown_cost; 255 is tested first.  Any other cell is blocked when cost >= lethal_cost and has cost' = cost
 *   otherwise.  A passable cell c weighs w(c) = neutral + cost'(c), 1..509.  Cells outside the grid are blocked.
 * Moves.  The 8 neighbours inside the grid.  A diagonal move is allowed only if both cells it squeezes between (the two that
 *   share an edge with both ends) are passable: no corner cutting.  Leaving cell b for a neighbour a costs k * w(b), k = 5 for
 *   a straight move and k = 7 for a diagonal one; both ends of a move are passable.
 * Potential, uint32 [n][gh][gw].  P(goal) = 0; for every other passable cell P(b) is the minimum over all allowed move
 *   sequences b -> ... -> goal of the summed move costs: the largest field with P(goal) = 0 and P(b) <= P(a) + k(a,b) * w(b)
 *   for every allowed move b -> a.  Blocked and unreachable cells hold 0xFFFFFFFF (SN_NAV_INF).
 *   uint32 suffices: gw * gh > 2^20 is refused (gw, gh 1..4096 each), a cheapest route visits no cell twice, so it leaves at
 *   most 2^20 - 1 cells, each at no more than 7 * (255 + 254) = 3563 (lethal_cost 255 lets a cell of 254 pass; 7 * 507 at
 *   the natural 253): (2^20 - 1) * 3563 = 3 736 072 725 < 2^32 - 1.  Every word the relaxation ever stores is the cost of
 *   such a route, and one further move added to it (3 736 076 288 at most) still fits.
 * Path (only with starts; written only with path and max_path > 0): start, c1, c2, ..., goal.  From cell c the next cell is
 *   the allowed neighbour a with the smallest P(a) + k(a,c) * w(c); ties go to the lowest index in the fixed order
 *   E, NE, N, NW, W, SW, S, SE (north is y - 1, east is x + 1).  w >= 1 makes P strictly decrease along the path, so it ends
 *   after fewer than gw * gh steps.  path int32 [n][max_path][2], {x, y} per cell; entries past the path's length are not
 *   written; a path longer than max_path leaves its first max_path cells and SN_NAV_PATH_TRUNCATED.  The walk is counted to its
 *   end whatever max_path is (stats reports the full length), one cell at a time by one wavefront per map, about a
 *   microsecond a cell: a route of a few hundred cells is a fraction of a millisecond, the longest route a 2^20-cell maze
 *   allows (some 5 * 10^5 cells) about half a second of one kernel.
 * stats uint32 [n][5] = {flags, passable cells with finite P, path length in cells (the full length even when truncated, and
 *   whether or not the path output is wanted; 0 without starts or without a route), P(start) or 0xFFFFFFFF (also without
 *   starts), blocked cells}.  flags:
 *   SN_NAV_GOAL_BLOCKED       the goal lies outside the grid or is blocked: every P is 0xFFFFFFFF and there is no path
 *   SN_NAV_START_UNREACHABLE  starts given, and the start lies outside the grid, is blocked, or has an infinite P
 *   SN_NAV_PATH_TRUNCATED     the path output is given and the path is longer than max_path (never without the output)
 *   SN_NAV_UNCONVERGED        max_rounds > 0 and work was left after the last round (see below)
 * potential, path and stats are each nullable, and at least one is required.
 * SN_ERR_ARG is decided before anything is launched or written (sn_last_error(h) names the call): a NULL h, p, cost or goals,
 *   n outside 1..max_batch, gw or gh outside 1..4096 or gw * gh > 2^20, neutral or lethal_cost outside 1..255, unknown_cost
 *   outside 0..252, flags with bits other than SN_NAV_UNKNOWN_OK, max_rounds or max_path negative, no output, path without
 *   starts or with max_path == 0, goals, starts, potential, path or stats not 4-byte aligned (cost may lie anywhere), any
 *   buffer overlapping another, a bad mem.
 * mem / stream as sn_inflate_grid: the stage has its own lane on the handle; a NULL stream is the lane's own (never the
 *   inference stream); calls are serialised by the lane's mutex and may run beside sn_submit / sn_wait and the other stages.
 * Rounds.  The field is relaxed tile by tile (SN_NAV_TILE_W x SN_NAV_TILE_H cells), one kernel launch per round.
 *   max_rounds == 0: the call runs until converged and returns after completion, whatever mem and stream are: the exact P,
 *     and SN_NAV_UNCONVERGED is never set.
 *   max_rounds > 0: exactly that many relaxation launches are enqueued and the host never waits in between; the call returns
 *     after completion when mem is SN_MEM_HOST or stream is NULL, and device buffers + a caller stream only enqueue, so
 *     obstacles -> costmap -> inflate -> navfn run on one stream without a host round trip.  If work was left after the last
 *     round SN_NAV_UNCONVERGED is set: every finite P is then the cost of a real route, an upper bound of the exact P, P
 *     still strictly decreases along the path, and the path still ends at the goal.
 *   rounds_out (host, nullable): how many rounds did work, for a call that returns after completion; -1 for one that only
 *     enqueues.  It depends on the schedule and belongs to no byte-for-byte comparison.
 * Not covered: the asynchronous sn_submit* slots, several goals per map, a goal tolerance (footprints with heading are
 * sn_rollout's, below), gradient-interpolated (sub-cell) paths, path smoothing, replanning from the previous frame's field. */
#define SN_NAV_TILE_W            32
#define SN_NAV_TILE_H            32
#define SN_NAV_MAX_CELLS         (1 << 20)   /* gw * gh */
#define SN_NAV_INF               0xFFFFFFFFu
#define SN_NAV_UNKNOWN_OK        1           /* params flags: a cell of 255 is passable at unknown_cost */
#define SN_NAV_GOAL_BLOCKED      1           /* stats flags */
#define SN_NAV_START_UNREACHABLE 2
#define SN_NAV_PATH_TRUNCATED    4
#define SN_NAV_UNCONVERGED       8
typedef struct sn_nav_params {
  int neutral;        /* 1..255: the price of a free cell */
  int lethal_cost;    /* 1..255: a cell with cost >= lethal_cost is blocked; 253 is the natural value */
  int unknown_cost;   /* 0..252: cost' of a cell of 255 under SN_NAV_UNKNOWN_OK */
  int flags;          /* SN_NAV_UNKNOWN_OK or 0 */
  int max_rounds;     /* >= 0; 0: until converged */
  int max_path;       /* >= 0: capacity of path per map, in cells */
} sn_nav_params;
int sn_navfn(sn_handle *h, int n, const uint8_t *cost /* [n][gh][gw] */, int gw, int gh, const int32_t *goals /* [n][2] */,
             const int32_t *starts /* [n][2], nullable */, const sn_nav_params *p, uint32_t *potential /* [n][gh][gw] */,
             int32_t *path /* [n][max_path][2] */, uint32_t *stats /* [n][5] */, int *rounds_out /* host, nullable */, int mem,
             void *stream);

/* ---- trajectory rollout: from the plan to a velocity command (csrc/sn_rollout.hpp; hobot_stereonet_amd/rollout.py is the numpy
 * twin, byte for byte) ----------------------------------------------------------------------------------------------------------
 * The local planner of a navigation stack (base_local_planner / DWA), directly after the navigation function: sample velocity
 * commands (v, w) on a fixed lattice, roll each forward along its constant-curvature arc for sim_time_s, reject the arcs on
 * which the robot's footprint touches an obstacle, score the rest by the cost-to-go at the arc's end and the worst cost under
 * the footprint, and take the cheapest.  sn_rollout does that for n maps: the cost grid of sn_inflate_grid, the potential of
 * sn_navfn over the same grid, one pose per map.  The stage is stateless.  All trigonometry is in two host-built tables and
 * the pose is quantised once on the host; everything below that is integer, so no tolerance appears anywhere.
 *
 * Samples.  S = nv * nw, sample s = iv * nw + iw, iv 0..nv-1, iw 0..nw-1.  The footprint is nf points {fx, fy} in metres in
 *   the robot's frame (x ahead, y to the left), 0 <= nf <= SN_ROLLOUT_MAX_POINTS; the robot's centre is always checked as well.
 * The host tables (sn_rollout_tables: pure host, no device), in double, in this order of operations, nothing contracted:
 *   k256 = 256.0 / (double)cell_m
 *   v(iv) = nv == 1 ? (double)v_min : (double)v_min + iv * (((double)v_max - (double)v_min) / (nv - 1)); w(iw) likewise
 *   for t = 0..T (T = steps):  tau = ((double)sim_time_s * t) / T;  th = w * tau;
 *     fabs(th) < 1e-6:  x = v * tau;  y = ((v * tau) * th) / 2;      otherwise  r = v / w;  x = r * sin(th);  y = r * (1 - cos(th))
 *     centres int32 [S][T+1][3] = {llrint(x * k256), llrint(y * k256), llrint((th / 6.283185307179586) * 65536) & 0xFFFF}
 *     offsets int32 [nw][T+1][nf][2] = {llrint((cos(th) * fx - sin(th) * fy) * k256), llrint((sin(th) * fx + cos(th) * fy) * k256)}
 *       with fx, fy widened to double first
 *   Either output may be NULL.  Two implementations of sin and cos may differ by an ulp, so an entry may differ by one between
 *   them: a twin is fed the library's tables, as it is fed sn_inflate_table's.
 *   SN_ERR_ARG: p NULL; cell_m, v_min, v_max, w_min, w_max or sim_time_s not finite; cell_m or sim_time_s <= 0; v_max < v_min or
 *   w_max < w_min; nv or nw outside 1..64; steps outside 1..SN_ROLLOUT_MAX_STEPS; lethal_cost or centre_lethal_cost outside
 *   1..255; unknown_cost outside 0..252; flags with bits other than SN_ROLLOUT_UNKNOWN_OK; w_goal or w_occ outside 0..32767 or
 *   both 0; nf outside 0..64, a NULL footprint with nf > 0, a footprint value that is not finite; fabs(th) above 2^20 at any
 *   step; any component of a centre, or of a centre plus an offset, above 2^21 in magnitude (8192 cells).
 * sn_rollout_pose_q (pure host): q[5] = {px, py, cq, sq, yaw_bam} of a pose {x, y, yaw} (metres and radians, in the frame the
 *   grid's origin is given in; origin = the outer corner of cell (0, 0)):  px = llrint((x - origin_x_m) * k256), py likewise:
 *   grid coordinates in 1/256 cell;  cq = llrint(cos(yaw) * 2^30), sq = llrint(sin(yaw) * 2^30);  yaw_bam =
 *   llrint((yaw / 6.283185307179586) * 65536) & 0xFFFF.  SN_ERR_ARG: a NULL pointer, cell_m not finite or <= 0, an origin or a
 *   pose value that is not finite, fabs(yaw) above 2^20, |px| or |py| above 2^30.
 * sn_rollout_velocity (pure host): out = {v(iv), w(iw)} of sample s as above; SN_ERR_ARG for parameters sn_rollout_tables
 *   refuses or s outside 0..S-1.
 *
 * Per map, sample and step t = 0..T, all integer, int64 where written, >> arithmetic (it floors):
 *   the centre is c = centres[s][t], footprint point f is c + offsets[iw][t][f], both {qx, qy} in 1/256 cell in the robot's frame
 *   at step 0;  X = px + (((int64)cq * qx - (int64)sq * qy + 2^29) >> 30),  Y = py + (((int64)sq * qx + (int64)cq * qy + 2^29) >> 30);
 *   the point lies in cell (X >> 8, Y >> 8).
 *   A point outside the grid collides.  A cell of 255 collides unless flags has SN_ROLLOUT_UNKNOWN_OK, and with it is priced at
 *   unknown_cost; 255 is tested first.  Any other cell collides when cost >= lethal_cost (a footprint point) or cost >=
 *   centre_lethal_cost (the centre), and is priced at its cost otherwise.
 *   A sample that collides anywhere has reason COLLISION, and its step is the smallest t at which any point collides.
 *   Otherwise occ = the largest price over all steps and points, and g = potential at the centre's cell at step T;
 *   g == SN_NAV_INF: reason NO_ROUTE.  Otherwise the sample is valid, score = (uint64)w_goal * g + (uint64)w_occ * occ < 2^48.
 *   window int32 [n][4] = {iv_lo, iv_hi, iw_lo, iw_hi}, inclusive (nullable: every sample): a sample outside it is not walked and
 *   has reason OUT_OF_WINDOW; an empty window is allowed.
 * Outputs, each nullable, at least one required:
 *   samples uint32 [n][S][2] = {g, info}: g is SN_NAV_INF unless the sample is valid; info = occ | reason << 8 | step << 16,
 *     occ 0 unless valid, step 0 unless COLLISION.
 *   best uint32 [n][8] = {flags, s_best, score_lo, score_hi, valid, collided, no_route, out_of_window}: the best sample is the
 *     valid one with the smallest score, ties to the lowest s (the minimum of the word score << 16 | s, the same in any order
 *     of reduction).  No valid sample: flags = SN_ROLLOUT_NO_VALID, s_best = score_lo = score_hi = 0xFFFFFFFF.  The four counts
 *     sum to S.
 *   traj int32 [n][T+1][3] = the best sample's centre per step, {X, Y, (yaw_bam + centres[s_best][t][2]) & 0xFFFF}: grid
 *     coordinates in 1/256 cell and the heading in 1/65536 turn.  A map without a valid sample keeps the caller's bytes.
 * SN_ERR_ARG is decided before anything is launched or written (sn_last_error(h) names the call): a NULL h, p, cost, potential
 *   or poses_q, n outside 1..max_batch, gw or gh outside 1..4096 or gw * gh > 2^20, anything sn_rollout_tables refuses, no
 *   output, potential, poses_q, window, samples, best or traj not 4-byte aligned (cost may lie anywhere), any buffer overlapping
 *   another, a bad mem.  poses_q is as sn_rollout_pose_q writes it (|px|, |py| <= 2^30, |cq|, |sq| <= 2^30); with other words
 *   nothing is read or written out of bounds, and the outputs mean nothing.
 * mem / stream as sn_navfn with fixed rounds (for a call whose tables are cached, see below): the stage has its own lane on the handle; poses_q and window are in the same
 *   memory kind as the grids, footprint is always host memory; the call returns after completion when mem is SN_MEM_HOST or
 *   stream is NULL; device buffers + a caller stream only enqueue, so inflate -> navfn (fixed rounds) -> rollout run on one
 *   stream without a host round trip.  May run beside sn_submit / sn_wait and the other stages.  Two kernel launches per call
 *   (one where samples alone is wanted).  The tables of the last (parameters, footprint) pair stay on the device: a call with
 *   the same pair builds and uploads nothing, one with another pair uploads its tables behind the lane's earlier calls and
 *   waits for the upload.
 * Not covered: the asynchronous sn_submit* slots, acceleration along the arc (each sample holds its velocity for the whole
 * of sim_time_s; sn_rollout's caller narrows the window to what the motors reach), path-distance and oscillation terms,
 * holonomic (sideways) samples, a score for rotation in place (such a sample ends where it began and is scored as that). */
#define SN_ROLLOUT_MAX_STEPS      64          /* steps (T) */
#define SN_ROLLOUT_MAX_POINTS     64          /* nf */
#define SN_ROLLOUT_MAX_SIDE       64          /* nv, nw */
#define SN_ROLLOUT_UNKNOWN_OK     1           /* params flags: a cell of 255 is priced at unknown_cost */
#define SN_ROLLOUT_NO_VALID       1           /* best flags */
#define SN_ROLLOUT_VALID          0           /* reasons */
#define SN_ROLLOUT_OUT_OF_WINDOW  1
#define SN_ROLLOUT_COLLISION      2
#define SN_ROLLOUT_NO_ROUTE       3
typedef struct sn_rollout_params {
  float cell_m;               /* > 0, finite: the grid's cell */
  float v_min, v_max;         /* m/s, v_min <= v_max */
  int   nv;                   /* 1..64 */
  float w_min, w_max;         /* rad/s, w_min <= w_max */
  int   nw;                   /* 1..64 */
  float sim_time_s;           /* > 0 */
  int   steps;                /* T, 1..SN_ROLLOUT_MAX_STEPS */
  int   lethal_cost;          /* 1..255: a footprint point collides when cost >= this; 254 is the natural value */
  int   centre_lethal_cost;   /* 1..255: the same for the centre; 253 is the natural value */
  int   unknown_cost;         /* 0..252: the price of a cell of 255 under SN_ROLLOUT_UNKNOWN_OK */
  int   flags;                /* SN_ROLLOUT_UNKNOWN_OK or 0 */
  int   w_goal, w_occ;        /* 0..32767 each, not both 0 */
} sn_rollout_params;
int sn_rollout_tables(const sn_rollout_params *p, const float *footprint /* [nf][2] */, int nf, int32_t *centres /* [S][T+1][3] */,
                      int32_t *offsets /* [nw][T+1][nf][2] */);                                         /* pure host, no device */
int sn_rollout_pose_q(float cell_m, double origin_x_m, double origin_y_m, const double *pose /* [3] */, int32_t *q /* [5] */);
int sn_rollout_velocity(const sn_rollout_params *p, int s, double *out /* [2] */);
int sn_rollout(sn_handle *h, int n, const uint8_t *cost /* [n][gh][gw] */, const uint32_t *potential /* [n][gh][gw] */, int gw,
               int gh, const int32_t *poses_q /* [n][5] */, const int32_t *window /* [n][4], nullable */, const sn_rollout_params *p,
               const float *footprint /* host [nf][2] */, int nf, uint32_t *samples /* [n][S][2] */, uint32_t *best /* [n][8] */,
               int32_t *traj /* [n][T+1][3] */, int mem, void *stream);

/* Measurement hook (bench.py --emulate-root-ingress): a device-to-device copy of `bytes` bytes by a kernel of exactly
 * `workgroups` workgroups of 256 threads on `stream` — the footprint of one RCCL receive (a few channels = a few
 * workgroups per peer), so that the tax of the gather root's ingress on a concurrently running batch can be measured
 * on one GPU.  dst / src: device pointers, 16-byte aligned; bytes a multiple of 16. */
int sn_dbg_copy_limited(void *dst, const void *src, size_t bytes, int workgroups, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* STEREONET_HIP_H_ */
