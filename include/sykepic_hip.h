/*
 * sykepic_hip.h — C-ABI of libsykepic_hip.so: the MI355X (gfx950) replacement
 * for the CNN classification hot path of sykefi/syke-pic.
 *
 * The reference has no FFI: its seam is Python duck-typing on three objects,
 * each created in exactly one place (paths relative to
 * /root/reference):
 *   - the network          sykepic/train/config.py:63-77  (TorchVisionNet(...))
 *   - the loss             sykepic/train/train.py:127     (nn.CrossEntropyLoss())
 *   - the optimizer        sykepic/train/train.py:131-138 (getattr(optim, name)([...]))
 * and everything heavy happens at two call sites:
 *   - inference  `out = net(x)` + base-1.3 softmax   sykepic/compute/probability.py:189-194
 *   - training   zero_grad/forward/loss/backward/step sykepic/train/train.py:239-243
 * Each entry point below names the reference lines it stands in for.  The
 * Python adapter (syke-pic_amd/sykepic_hip/lib.py) binds them with ctypes.
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer it
 * passes; the library owns weights, activations, gradients and workspace
 * inside the handle; no exception crosses the boundary (0 = ok, <0 = error,
 * text via spk_last_error()).  Host-facing parameter I/O always uses the
 * reference's on-disk layout (NCHW / [out,in] float32, int64 counters) so a
 * best_state.pth stays interchangeable.  Device pointers are HIP device
 * memory on the model's device; work is enqueued on the model's stream
 * (spk_model_set_stream) and is asynchronous unless stated.
 */
#ifndef SYKEPIC_HIP_H
#define SYKEPIC_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPK_OK 0
#define SPK_ERR_ARG (-1)
#define SPK_ERR_HIP (-2)
#define SPK_ERR_KEY (-3)
#define SPK_ERR_UNSUPPORTED (-4)
#define SPK_ERR_STATE (-5)

/* layer kinds of spk_layer_desc.kind */
#define SPK_OP_CONV 1      /* Conv2d(bias=False) + BatchNorm2d (+residual) (+ReLU) */
#define SPK_OP_MAXPOOL 2   /* MaxPool2d(k, stride, pad) */
#define SPK_OP_GAVGPOOL 3  /* AdaptiveAvgPool2d(1) + flatten */
#define SPK_OP_LINEAR 4    /* Linear with bias, no activation (head) */
#define SPK_OP_DROPOUT 5   /* Dropout(p) in the head */
/* EfficientNet and MobileNetV3 (torchvision MBConv / InvertedResidual; eval and training):
 *   DWCONV: depthwise Conv2d(C, C, k, stride, pad=(k-1)/2, groups=C, bias=False) + BatchNorm2d + activation
 *   SE:     SqueezeExcitation(C, squeeze = `k`): avgpool -> fc1 (1x1 conv, bias) -> act1 -> fc2 -> act2 -> x * s;
 *           `name` is the module prefix (name.fc1.weight ...), cin = cout = C.  `relu` names the gate pair:
 *           0 = SiLU, Sigmoid (EfficientNet); SPK_ACT_RELU = ReLU, Hardsigmoid (MobileNetV3); any other value is
 *           SPK_ERR_UNSUPPORTED at create. */
#define SPK_OP_DWCONV 6
#define SPK_OP_SE 7

/* spk_layer_desc.relu: activation after BatchNorm (+ residual) */
#define SPK_ACT_NONE 0
#define SPK_ACT_RELU 1
#define SPK_ACT_SILU 2
#define SPK_ACT_HSWISH 3  /* Hardswish x * clamp(x + 3, 0, 6) / 6 (MobileNetV3; CONV and DWCONV layers) */

/* input layouts / dtypes of the image batch */
#define SPK_LAYOUT_NCHW 0
#define SPK_LAYOUT_NHWC 1
#define SPK_DTYPE_F32 0
#define SPK_DTYPE_I64 1
#define SPK_DTYPE_U8 2

/* optimizers (reference: `getattr(optim, name)` with only `lr` given, sykepic/train/train.py:131-138; Adam is the
 * default, train.ini.example:74): the first-order torch.optim classes with their torch default hyper-parameters */
#define SPK_OPT_SGD 0
#define SPK_OPT_ADAM 1
#define SPK_OPT_ADAMW 2     /* decoupled weight decay (default 0.01) */
#define SPK_OPT_RMSPROP 3   /* alpha 0.99, eps 1e-8, optional momentum; centered = False */
#define SPK_OPT_ADAGRAD 4   /* lr_decay, initial_accumulator_value, eps 1e-10 */
#define SPK_OPT_ADAMAX 5
#define SPK_OPT_NADAM 6     /* momentum_decay 4e-3 */
#define SPK_OPT_RADAM 7
#define SPK_OPT_ADADELTA 8  /* rho 0.9, eps 1e-6 */
#define SPK_OPT_ASGD 9      /* lambd 1e-4 (field lr_decay), alpha 0.75 (field alpha), t0 1e6; the averaged copy `ax` is not kept */
#define SPK_OPT_RPROP 10    /* etas (0.5, 1.2) in beta1 / beta2, step sizes (1e-6, 50) in eps / alpha */

typedef struct spk_model spk_model;

/* One node of the layer graph that TorchVisionNet.__init__ builds
 * (sykepic/train/network.py:48-63): backbone children minus the last one,
 * then the Linear head.  `name`/`bn` are state_dict prefixes ("base.4.0.conv1",
 * "base.4.0.bn1", "head.0"). src/dst/res are activation ids (0 = input). */
typedef struct {
  int32_t kind;
  int32_t cin, cout, k, stride, pad;
  int32_t relu;  /* SPK_ACT_* */
  int32_t src, dst, res;
  int32_t child; /* index of the owning child of `base`; -1 for the head */
  float p;       /* dropout probability */
  char name[96];
  char bn[96];
} spk_layer_desc;

/* Hyper-parameters of one optimizer step; lr per param group as kept by
 * LRWarmup (sykepic/train/network.py:98-130). */
typedef struct {
  int32_t kind;     /* SPK_OPT_* */
  float lr[3];
  float beta1, beta2, eps;  /* Adam */
  float weight_decay;
  float momentum;           /* SGD, RMSprop */
  float grad_scale;         /* multiplies every gradient first (1/world for DP mean) */
  float alpha;              /* RMSprop smoothing constant / Adadelta rho */
  float momentum_decay;     /* NAdam */
  float lr_decay;           /* Adagrad */
  float initial_accumulator_value; /* Adagrad */
} spk_optim_desc;

const char* spk_last_error(void);
const char* spk_version(void);

/* TorchVisionNet(...) construction — sykepic/train/config.py:63-77,
 * sykepic/train/network.py:14-64.  Weights start at zero; load them with
 * spk_model_load_param. */
int spk_model_create(const spk_layer_desc* layers, int n_layers, int in_chans,
                     int num_classes, int device, spk_model** out);
/* The same with one Conv2d `groups` value per layer (torchvision ResNeXt: conv2 of every bottleneck has groups > 1);
 * groups == NULL is spk_model_create.  A layer with groups > 1 must be a conv with k 3, pad 1, stride 1 or 2,
 * cin == cout a multiple of 16 and 4, 8, 16, 32 or 64 channels per group, no shortcut operand and no activation but
 * ReLU (else SPK_ERR_UNSUPPORTED).  Its weight tensor is [cout][cin / groups][k][k], as in the state_dict. */
int spk_model_create_grouped(const spk_layer_desc* layers, const int32_t* groups, int n_layers, int in_chans,
                             int num_classes, int device, spk_model** out);
void spk_model_destroy(spk_model* m);
/* net.to(device) has no counterpart (the handle lives on one GPU); the
 * stream is a hipStream_t (0 = default stream). */
int spk_model_set_stream(spk_model* m, void* hip_stream);

/* state_dict()/load_state_dict() — sykepic/train/train.py:300,179,
 * sykepic/compute/probability.py:129.  Enumerates tensors in torch's
 * state_dict order. dtype is SPK_DTYPE_F32 or SPK_DTYPE_I64
 * (num_batches_tracked). Synchronous. */
int spk_model_num_params(spk_model* m);
int spk_model_param_info(spk_model* m, int idx, char* key, int key_cap,
                         int64_t shape[4], int* ndim, int* dtype);
int spk_model_load_param(spk_model* m, const char* key, const void* host, int64_t numel);
int spk_model_read_param(spk_model* m, const char* key, void* host, int64_t numel);

/* param.requires_grad = flag — sykepic/train/network.py:133-172 */
int spk_model_set_requires_grad(spk_model* m, const char* key, int flag);
/* optimizer.param_groups[group]["params"] membership (group -1: not in the
 * optimizer) — sykepic/train/train.py:131-138, network.py:108-128 */
int spk_model_set_param_group(spk_model* m, const char* key, int group);
/* 16-bit storage/MFMA input type of the eval path: 0 = fp16 (default; the
 * 1e-3 probability tolerance needs its 11-bit mantissa), 1 = bf16. fp32
 * accumulation either way. Training always runs bf16. */
int spk_model_set_infer_dtype(spk_model* m, int bf16);
/* Precision knobs of the fp16 eval path (defaults: split_weights = 3,
 * precise_residual = 0).  split_weights = 2 splits only the convs that write
 * the residual trunk (stem, block-closing convs, downsample branches);
 * split_weights = 3 splits every conv except the 3x3 convs inside a residual
 * block (the lo-products that buy the least accuracy per MFMA cycle) - and, on
 * the EfficientNet graphs, no conv at all: their error is the fp16 rounding of
 * the stored activations, the weight rounding does not show beside it
 * (tests/archive/diagnostics/effnet_calibrated.py; 1 still splits every conv).
 * split_weights = 1: every conv weight is carried as
 * hi + lo fp16 halves and both products are accumulated (2x MFMA work, weight
 * rounding error ~2^-22) — weight rounding is the dominant logit error at
 * 16-bit storage.  MobileNetV3 graphs (Hardswish / Hardsigmoid): split_weights = 3
 * splits every conv, and split_weights = 5 returns SPK_ERR_UNSUPPORTED.  precise_residual: shortcut tensors keep their fp16
 * rounding remainder for the residual add (+2 B/element of shortcut traffic). */
int spk_model_set_precision(spk_model* m, int split_weights, int precise_residual);
/* Per-op choice of split weights: flags[i] != 0 carries conv op i (index into the
 * spk_layer_desc array of spk_model_create) as hi+lo halves; flags of non-conv ops
 * are ignored.  Replaces the split_weights mode until spk_model_set_precision is
 * called again.  `tests/archive/diagnostics/split_search.py` derives the cheapest mask that keeps
 * the reference's 1e-3 probability tolerance. */
int spk_model_set_split_ops(spk_model* m, const unsigned char* flags, int n_ops);
/* Calibrated single-pass mode (round 4): split_weights = 5 in spk_model_set_precision.
 * An fp16 weight image loses dw = fp16(w) - w per weight and an output loses sum_k dw_k x_k; over the data that error has
 * a mean, sum_k dw_k E[x_k], the same for every pixel of an output channel - and this systematic part is most of the
 * logit error of a plain fp16 forward.  With per-channel means E[x_k] of every conv's input, each weight row (per filter
 * tap) is rounded to nearest and then the weights nearest a rounding midpoint are re-rounded until sum_k E[x_k] dw_k ~ 0
 * ("zero-sum rounding", csrc/zero_sum.hip): the mean error is gone at no run-time cost, the row's squared error grows
 * by < 1 %.  Mode 5 runs every conv as ONE fp16 product (the 7x7 stem too: its 147-weight rows are balanced as a whole
 * against the image's own channel means) and needs the means:
 *   spk_model_calibrate_act_means - one batch of representative images (as spk_forward_infer takes them) through the
 *     most accurate mode; per-channel means of every conv input, accumulated over calls (reset != 0 starts over);
 *   spk_model_get_act_means / spk_model_set_act_means - the flat vector (spk_model_act_means_size floats: cin values
 *     per conv, graph order) to store with the model and restore (`act_means.pth` next to
 *     `best_state.pth`); set with host == NULL forgets them;
 *   spk_model_set_zero_sum - apply the rounding to the un-split convs of ANY split mode (diagnostics).
 * A model's probabilities stay a function of (weights, means, image): nothing depends on the batch an image arrives in.
 * spk_forward_infer in mode 5 without means fails with SPK_ERR_STATE.  Reference call site: `net(x)`,
 * sykepic/compute/probability.py:189. */
int64_t spk_model_act_means_size(spk_model* m);
int spk_model_calibrate_act_means(spk_model* m, const void* x_dev, int n, int h, int w, int layout, int dtype, int reset);
int spk_model_get_act_means(spk_model* m, float* host, int64_t numel);
int spk_model_set_act_means(spk_model* m, const float* host, int64_t numel);
int spk_model_set_zero_sum(spk_model* m, int on);
/* fp8 (OCP e4m3) eval mode of the EfficientNet MBConv blocks — BASELINE config 5.  Inside a block (expand 1x1
 * conv -> depthwise conv -> squeeze-excitation -> project 1x1 conv) the expanded tensors are stored as e4m3
 * bytes with one scale per tensor, the 1x1 convs run on the fp8 MFMA with e4m3 weights (one scale per output
 * channel) and the squeeze-excitation gate is applied in the project conv's operand loader; the residual
 * trunk, the stem, the head and any block without an expand conv stay fp16.  spk_model_calibrate_fp8 runs one
 * fp16 forward of a representative device batch (as spk_forward_infer takes it) and records the activation
 * ranges; it must be called before the first fp8 forward and again after loading other weights.  3 mantissa
 * bits do not reach the 1e-3 probability tolerance of the reference: the fp16 path stays the parity mode. */
/* A graph with a Hardswish layer or a ReLU / Hardsigmoid squeeze-excitation gate (MobileNetV3) has no fp8 mode:
 * spk_model_set_fp8(m, 1) returns SPK_ERR_UNSUPPORTED. */
int spk_model_set_fp8(spk_model* m, int on);
int spk_model_calibrate_fp8(spk_model* m, const void* x_dev, int n, int h, int w, int layout, int dtype);
/* Which MBConv blocks the fp8 mode covers (round 3).  Blocks are counted in graph order over those that qualify
 * (expand conv -> depthwise -> squeeze-excitation -> project conv); flags[i] != 0 puts block i on the e4m3 path, 0 keeps
 * it fp16.  n_blocks = 0 (or never calling this) selects the default set: every qualifying block that has a
 * shortcut (a block without one replaces the trunk by its e4m3-computed output and costs most of the accuracy).  Takes
 * effect at the next spk_model_calibrate_fp8.  spk_model_num_fp8_blocks returns how many blocks qualify. */
int spk_model_set_fp8_blocks(spk_model* m, const unsigned char* flags, int n_blocks);
int spk_model_num_fp8_blocks(spk_model* m);
/* BatchNorm2d(eps, momentum) of every BatchNorm in the graph: torch's defaults 1e-5 / 0.1 unless the model family says
 * otherwise (torchvision's efficientnet_b5..b7 are built with eps 1e-3, momentum 0.01). */
int spk_model_set_bn(spk_model* m, float eps, float momentum);
/* Dropout mask seed for training steps. */
int spk_model_set_seed(spk_model* m, uint64_t seed);

/* net.eval(); out = net(x); softmax(out * ln(base)) — the body of net_pass,
 * sykepic/compute/probability.py:184-194.  x: n images h x w of the model's
 * in_chans; out: float32 [n, num_classes] device buffer.  softmax_base <= 0
 * returns raw logits (test_net / val loop, sykepic/train/train.py:265,338). */
int spk_forward_infer(spk_model* m, const void* x_dev, int n, int h, int w, int layout,
                      int dtype, float softmax_base, float* out_dev);

/* net.eval() forward + CrossEntropyLoss + arg-max accuracy — the validation
 * loop body, sykepic/train/train.py:262-270.  stats_dev: float32[2] device
 * buffer, ACCUMULATED: stats[0] += loss*n, stats[1] += #correct.  logits_dev
 * may be NULL. */
int spk_eval_step(spk_model* m, const void* x_dev, int n, int h, int w, int layout, int dtype,
                  const int64_t* y_dev, float* stats_dev, float* logits_dev);

/* net.train(); optimizer.zero_grad(); out = net(x); loss = CE(out, y);
 * loss.backward() — sykepic/train/train.py:233,239-242.  Train-mode BatchNorm
 * (batch statistics, running-stat update, num_batches_tracked += 1).
 * Gradients land in the flat buffer of spk_model_grad_buffer; stats_dev as
 * in spk_eval_step (train.py:244-247). */
int spk_train_forward_backward(spk_model* m, const void* x_dev, int n, int h, int w, int layout,
                               int dtype, const int64_t* y_dev, float* stats_dev,
                               float* logits_dev);
/* The same step with the Mixup / CutMix criterion on a batch mixed by spk_mix_batch (not in the reference, whose loop
 * is train.py:239-242): loss = lam CE(out, ya) + (1 - lam) CE(out, yb), CE the model's loss (spk_model_set_loss: its
 * weights and smoothing; none and 0 for the default one), each term normalised by its own sum of weights, 1 - lam
 * formed in float32.  stats[0] += n * loss; stats[1] and the per-class counters (kept exactly when the loss keeps
 * them) count against the dominant label, ya when lam >= 0.5, else yb.  yb_dev == NULL or lam == 1:
 * spk_train_forward_backward on ya, bit for bit, whatever the loss.  Checked before any HIP call: a null m / x_dev /
 * ya_dev / stats_dev, n < 1, lam outside [0, 1] or not finite are SPK_ERR_ARG. */
int spk_train_forward_backward_pair(spk_model* m, const void* x_dev, int n, int h, int w, int layout, int dtype,
                                    const int64_t* ya_dev, const int64_t* yb_dev, float lam,
                                    float* stats_dev, float* logits_dev);
/* The same step with knowledge distillation from a teacher (not in the reference): teacher_logits_dev is a float32
 * [n][num_classes] device buffer of the teacher's logits for this very batch, and
 *   loss = (1 - alpha) L_hard + alpha T^2 KL(softmax(teacher / T) || softmax(out / T))      ("batchmean", T = temperature)
 * with L_hard the loss of spk_train_forward_backward_pair (one or two label vectors, the model's weights and smoothing),
 * 1 - alpha formed in float32.  stats[0] += n * loss; stats[1] and the per-class counters as in the pair step.
 * kd_stats_dev (may be NULL): float32 [2], [0] += n * KD (the KL term with its T^2), [1] += rows whose arg-max equals
 * the teacher's (lowest index among the maxima on both sides).  teacher_logits_dev == NULL or alpha == 0:
 * spk_train_forward_backward_pair, bit for bit; the teacher is not read and kd_stats_dev not written.  Checked before
 * any HIP call: what the pair step checks, alpha outside [0, 1], temperature not finite or <= 0, and a kd_stats_dev
 * without teacher_logits_dev are SPK_ERR_ARG. */
int spk_train_forward_backward_distill(spk_model* m, const void* x_dev, int n, int h, int w, int layout, int dtype,
                                       const int64_t* ya_dev, const int64_t* yb_dev, float lam,
                                       const float* teacher_logits_dev, float alpha, float temperature,
                                       float* stats_dev, float* kd_stats_dev, float* logits_dev);
/* optimizer.step() — sykepic/train/train.py:243 */
int spk_optim_step(spk_model* m, const spk_optim_desc* opt);

/* Flat float32 gradient buffer covering every trainable tensor (device
 * pointer, element count): what a data-parallel caller all-reduces over RCCL
 * between spk_train_forward_backward and spk_optim_step. */
int spk_model_grad_buffer(spk_model* m, void** dev_ptr, int64_t* numel);
/* Data-parallel overlap: the flat gradient buffer is produced back to front (head and layer4 first, the stem
 * last).  With a callback installed, spk_train_forward_backward reports each contiguous slice [offset, offset +
 * numel) of the buffer as soon as every kernel that writes it has been ENQUEUED: it records an event on the
 * model's stream, makes `comm_stream` (a hipStream_t) wait for it, then calls cb(user, bucket, offset, numel)
 * on the calling host thread.  The callee starts its collective on `comm_stream` (torch: `dist.all_reduce(view,
 * async_op=True)` under `torch.cuda.stream(comm)`), which then runs beside the rest of the backward pass.
 * n_buckets 1..3 (slices: head + last stage | the stage before | everything earlier); cb == NULL removes it. */
typedef void (*spk_grad_ready_fn)(void* user, int bucket, int64_t offset, int64_t numel);
int spk_model_set_grad_ready_callback(spk_model* m, spk_grad_ready_fn cb, void* user, void* comm_stream,
                                      int n_buckets);
/* Gradient of one tensor, copied to host in state_dict layout (tests). */
int spk_model_read_grad(spk_model* m, const char* key, void* host, int64_t numel);

/* --- Checkpointing a training run (resume; the reference saves the weights alone, sykepic/train/train.py:300) ---
 * Everything the next spk_train_forward_backward + spk_optim_step reads that is neither a parameter nor a buffer of
 * the state_dict, a hyper-parameter of spk_optim_desc, the group / requires_grad flags (set by key above) nor the
 * input batch:
 *   - the two moment buffers of the optimizer kernels, per tensor (slot 0 / 1; which torch.optim state entry each holds
 *     depends on the optimizer kind: SGD momentum_buffer / -; Adam, AdamW, NAdam, RAdam exp_avg / exp_avg_sq; Adamax
 *     exp_avg / exp_inf; RMSprop momentum_buffer / square_avg; Adagrad - / sum; Adadelta square_avg / acc_delta;
 *     Rprop prev / step_size; ASGD none)
 *   - per tensor: the step count (bias corrections, "first step" initialisations, Adagrad / ASGD / RAdam schedules)
 *     and NAdam's running mu product (kept in double)
 *   - per model: the number of training steps so far and the seed, which together with the layer index select the
 *     Dropout and stochastic-depth masks of a step
 * Nothing else survives a step: gradients, batch statistics, masks and the packed bf16 weight images are rebuilt by
 * every step (the images whenever a parameter was loaded or stepped), the side-stream bookkeeping is joined by every
 * reader, and the `sgd_started` flag of the training state is never read (a tensor's first step is step == 1).
 *
 * Moments of one tensor, float32 in state_dict layout (OIHW for conv weights) like spk_model_read_param: the state
 * `optimizer.step()` (train.py:243) keeps for `getattr(optim, name)(groups)` (train.py:131-138).  Synchronous.  Before
 * any training step a read returns zeros; a load creates the training state.  Unknown key: SPK_ERR_KEY; a buffer
 * (no gradient), a size mismatch or a slot other than 0 / 1: SPK_ERR_ARG. */
int spk_model_optim_state_read(spk_model* m, const char* key, int slot, float* host, int64_t numel);
int spk_model_optim_state_load(spk_model* m, const char* key, int slot, const float* host, int64_t numel);
/* Per-tensor counters of optimizer.step() (train.py:243): torch's state["step"] as an exact integer and NAdam's
 * state["mu_product"] (1.0 for every other optimizer and before the first step). */
int spk_model_param_counters_get(spk_model* m, const char* key, int64_t* step, double* mu_product);
int spk_model_param_counters_set(spk_model* m, const char* key, int64_t step, double mu_product);
/* Per-model counters: training steps run so far (spk_train_forward_backward calls, train.py:239-242) and the mask
 * seed of spk_model_set_seed.  The setter creates the training state. */
int spk_model_train_counters_get(spk_model* m, uint64_t* steps, uint64_t* seed);
int spk_model_train_counters_set(spk_model* m, uint64_t steps, uint64_t seed);

/* loss_fn = nn.CrossEntropyLoss(weight, label_smoothing) (sykepic/train/train.py:127) for spk_train_forward_backward
 * AND spk_eval_step (the reference validates with the same loss_fn).  class_weights_host: float32 [num_classes] or NULL
 * (all ones).  Checked before any HIP call: a weight that is not finite or not above 0, or a label_smoothing outside
 * [0, 1], is SPK_ERR_ARG.  With weights or label_smoothing > 0 the steps run the weighted / smoothed kernel, stats[0]
 * accumulates n * loss of that loss, and the per-class counters below are kept; (NULL, 0) - the state of a new
 * handle - returns to the plain kernel, bit for bit.  Synchronous. */
int spk_model_set_loss(spk_model* m, const float* class_weights_host, float label_smoothing);
/* Per class (rows seen, rows correct) over the training and validation steps since the last reset, int64
 * [num_classes][2]; reset != 0 zeroes the counters after the read.  SPK_ERR_UNSUPPORTED while the loss is the default
 * one (no counters are kept).  Synchronous. */
int spk_model_class_counts_read(spk_model* m, int64_t* host, int reset);

/* --- Exponential moving average (EMA) of the weights (not in the reference; the usual fine-tuning recipe) ---
 * A second flat float32 buffer in the layout of the model's own: every parameter and every float buffer (BatchNorm
 * running mean / variance).  num_batches_tracked (int64) is not averaged: the model's own value serves both states.
 * Every argument and state check happens before any HIP call.
 *
 * spk_model_ema_enable(m, on != 0): allocate the buffer (4 bytes per flat element) and copy the model's tensors into
 *   it - the average STARTS as a copy; enabled already: copy again.  SPK_ERR_STATE while swapped in.  on == 0: free it; an
 *   average that is swapped in is swapped out first, so the model keeps its own weights.  spk_model_destroy frees it.
 *   Synchronous.
 * spk_model_ema_update(m, w): avg[i] = fma(w, model[i] - avg[i], avg[i]) over the whole buffer - one fused multiply-add
 *   of the float32-rounded difference, torch.lerp's formula for w < 0.5, used here for every w; w = 1 - decay.  Where
 *   model[i] == avg[i] the average keeps its bits (a frozen tensor's average stays the tensor), except that -0 becomes
 *   +0.  One launch on the model's stream, behind everything the last training and optimizer step left running.
 *   w not finite or outside (0, 1): SPK_ERR_ARG; not enabled, or swapped in: SPK_ERR_STATE.
 * spk_model_ema_swap(m): exchange the CONTENTS of the two buffers (one launch on the model's stream; pointers and
 *   offsets stay) and toggle the `swapped` state; every packed weight image is rebuilt from what the model's buffer
 *   now holds.  While swapped in, spk_eval_step, spk_forward_infer, spk_model_read_param and spk_model_load_param work
 *   on the average, spk_train_forward_backward*, spk_optim_step and spk_model_ema_update return SPK_ERR_STATE ("the
 *   moving average is swapped in"), and spk_model_ema_read / _load address the model's own tensors.  Not enabled:
 *   SPK_ERR_STATE.
 * spk_model_load_param on a model that is NOT swapped in changes the model alone: the average keeps its values
 *   (spk_model_ema_load, or spk_model_ema_enable again, sets them).
 * spk_model_ema_read / spk_model_ema_load: one float tensor of the other buffer, float32 in state_dict layout like
 *   spk_model_read_param.  Synchronous.  A null argument, an int64 key or a size mismatch: SPK_ERR_ARG; unknown key:
 *   SPK_ERR_KEY; not enabled: SPK_ERR_STATE.
 * spk_model_ema_state: the two flags. */
int spk_model_ema_enable(spk_model* m, int on);
int spk_model_ema_update(spk_model* m, float w);
int spk_model_ema_swap(spk_model* m);
int spk_model_ema_read(spk_model* m, const char* key, float* host, int64_t numel);
int spk_model_ema_load(spk_model* m, const char* key, const float* host, int64_t numel);
int spk_model_ema_state(spk_model* m, int* enabled, int* swapped);
/* Test hooks: the launches of spk_model_ema_update / spk_model_ema_swap on caller buffers, n floats each at any 4-byte
 * aligned device address (16-byte accesses on the aligned body, element accesses on the head and the tail).
 * Synchronous.  SPK_ERR_ARG, before any HIP call: a null pointer, n < 1, a misaligned pointer, overlapping ranges, w not
 * finite or outside (0, 1). */
int spk_op_ema_lerp(float* e_dev, const float* p_dev, int64_t n, float w, void* hip_stream);
int spk_op_swap_f32(float* a_dev, float* b_dev, int64_t n, void* hip_stream);

/* Test hook: copy activation `tensor_id` (spk_layer_desc.dst numbering) of the
 * most recent forward to the host as float32 NCHW ([n,c,h,w]; [n,c] for the
 * head).  The stem input (id 0) is not readable.  Synchronous. */
int spk_model_read_activation(spk_model* m, int tensor_id, int n, float* host, int64_t numel);

/* Test hook: gradient w.r.t. activation `tensor_id` left by the most recent
 * spk_train_forward_backward, float32 NCHW like spk_model_read_activation. */
int spk_model_read_activation_grad(spk_model* m, int tensor_id, int n, float* host, int64_t numel);

/* --- Test hooks: single operators of the training step on caller-provided device buffers ---
 * What `out = net(x)` (train mode) and `loss.backward()` run for ONE Conv2d+BatchNorm2d layer
 * (sykepic/train/train.py:240,242): the same launches spk_train_forward_backward makes, so that a parity
 * test can hand a kernel known operands and compare with torch autograd on the same bf16-rounded operands.
 * Activations / gradients: NHWC bf16 device buffers (the 7x7/2 stem input: 4 stored channels, even width);
 * weights and weight gradients: float32 [Cout][kh][kw][Cin] device buffers; h, w are the conv INPUT size.
 * Channel counts: multiples of 64 (stem: cin <= 4, cout 64).  Synchronous (the call returns after the work).
 *
 * conv -> batch statistics -> normalise (+res) (+ReLU).  raw: conv output before BatchNorm (bf16);
 * mask: one ReLU bit per element ([M][C/8] bytes; may be NULL when relu == 0); mean_invstd: float[2][C];
 * running_mean / running_var are updated in place (momentum 0.1, unbiased variance). */
int spk_op_conv_bn_train_forward(const void* x_dev, const float* w_dev, const float* gamma_dev, const float* beta_dev,
                                 float* running_mean_dev, float* running_var_dev, const void* res_dev, void* out_dev,
                                 void* raw_dev, unsigned char* mask_dev, float* mean_invstd_dev, int n, int h, int w,
                                 int cin, int cout, int k, int stride, int pad, int relu, void* hip_stream);
/* BatchNorm2d (+ReLU) backward: g = gradient w.r.t. the layer output [M][C]; dy = gradient w.r.t. the conv output;
 * g_res (optional) receives (or, res_accumulate != 0, adds) the gradient of the shortcut operand;
 * dgamma / dbeta: float[C] (either may be NULL). */
int spk_op_bn_backward(const void* g_dev, const unsigned char* mask_dev, const void* raw_dev, const float* mean_dev,
                       const float* invstd_dev, const float* gamma_dev, float* dgamma_dev, float* dbeta_dev,
                       void* dy_dev, void* g_res_dev, int res_accumulate, int m_rows, int channels, int relu,
                       void* hip_stream);
/* Conv2d data gradient: dx [n,h,w,cin] (= or, accumulate != 0, +=) conv_transpose(dy [n,ho,wo,cout], w). */
int spk_op_conv_dgrad(const void* dy_dev, const float* w_dev, void* dx_dev, int accumulate, int n, int h, int w,
                      int cin, int cout, int k, int stride, int pad, void* hip_stream);
/* Data gradient of a STRIDE-1 conv + the BatchNorm backward of the layer that produced the conv's input, as a training step
 * runs them since round 4: the dgrad epilogue makes that BatchNorm's per-channel sums (sum dz, sum dz * xhat) from the fp32
 * gradient values it is about to store, so the producer's reduce pass is skipped (csrc/conv_igemm.hip, spk_set_bnb).
 * dx (+)= conv_transpose(dy, w) [n,h,w,cin] bf16; raw / mask / mean / invstd / gamma describe the producer ([n,h,w,cin] bf16
 * raw output, one ReLU bit per element, [cin] floats); dy_prod = gradient of the producer's raw output, dgamma / dbeta [cin].
 * res_src / res_bits (both or neither, instead of accumulate): the shortcut gradient picked up at its source - dx =
 * conv_transpose(dy, w) + res_src * bit, res_src [n,h,w,cin] bf16 = the output gradient of the block-closing conv whose
 * shortcut this tensor is, res_bits its ReLU bits - so that its BatchNorm backward need not write it into dx first.
 * Reference: loss.backward(), sykepic/train/train.py:242. */
int spk_op_conv_dgrad_bn_backward(const void* dy, const float* w_ohwi, void* dx, int accumulate, const void* raw,
                                  const unsigned char* mask, const float* mean, const float* invstd, const float* gamma,
                                  float* dgamma, float* dbeta, void* dy_prod, int n, int h, int w, int cin, int cout, int k,
                                  int pad, int relu, const void* res_src, const unsigned char* res_bits, void* stream);
/* Pins the implicit-GEMM candidate (csrc/conv_igemm.hip) of every later convolution of the process: tile config
 * cfg 0..6 with main-loop flavour dma 0..6 (0 register-staged, 1 LDS-DMA 3-4 stage, 3 LDS-DMA 2 stage, 4 hybrid,
 * 5 BK-32, 6 one stage), and the weight-gradient pipeline depth wgrad_nbuf 1 / 2 (csrc/conv_wgrad.hip).  -1 in a field:
 * not pinned, the tuner decides as without the call (cfg and dma are pinned together or not at all).  A pinned launch
 * reads and appends nothing of the tune cache and runs exactly that candidate; the single-operator hooks above and
 * spk_op_conv1x1 / spk_op_conv3x3 (cfg < 0) fail with SPK_ERR_UNSUPPORTED ("does not fit") when the flavour is not
 * instantiated for the problem's tile (configs 5 -> 4 -> 3 are still narrowed when Cout % 256 / % 128).  For tests. */
int spk_op_conv_pin(int cfg, int dma, int wgrad_nbuf);
/* The tuner table of the process (csrc/tune_table.h) by the tag of a tune-cache line: "conv", "pw1x1", ... and the
 * paired siblings "conv_p", ... that the half batches of a two-stream eval forward are tuned under.  what 0: looks the
 * key up (exact, else the nearest tuned batch), *found = 1 and vals filled, or *found = 0; what 1: stores vals for the
 * key and appends the line to the SPK_TUNE_CACHE file; what 2: forgets every entry, the next call reads the file again
 * (tag, key and vals are not used).  n_key / n_vals must be the tag's field counts.  No HIP call.  For tests. */
int spk_op_tune_table(int what, const char* tag, const int* key, int n_key, int* vals, int n_vals, int* found);
/* Conv2d weight gradient: dw [Cout][kh][kw][Cin] float32 from x [n,h,w,cin] and dy [n,ho,wo,cout]. */
int spk_op_conv_wgrad(const void* x_dev, const void* dy_dev, float* dw_dev, int n, int h, int w, int cin, int cout,
                      int k, int stride, int pad, void* hip_stream);
/* Grouped 3x3 pad-1 convolution, stride 1 or 2 (csrc/conv_group.hip: the conv2 of a ResNeXt bottleneck, Conv2d(c, c, 3,
 * stride, 1, groups) in `net(x)` and in the training step, sykepic/train/train.py:240,242).  NHWC activations, fp32 weights
 * and weight gradients [c][3][3][c / groups] (as the other single-operator hooks: input channel innermost); h, w are the conv INPUT size; c a multiple of 16 and
 * 4 / 8 / 16 / 32 / 64 channels per group, else SPK_ERR_UNSUPPORTED.  Synchronous.
 * spk_op_conv_group: y = relu?(conv * bn_scale + bn_bias), x / y fp16 (bf16 == 0) or bf16; bn_scale == bn_bias == NULL:
 *   the raw conv output, as the training forward stores it before its BatchNorm.
 * spk_op_conv_group_dgrad: dx [n,h,w,c] (= or, accumulate != 0, +=) conv_transpose(dy), bf16.
 * spk_op_conv_group_wgrad: dw from x [n,h,w,c] and dy [n,ho,wo,c], bf16. */
int spk_op_conv_group(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                      void* y_dev, int n, int h, int w, int c, int groups, int stride, int relu, int bf16,
                      void* hip_stream);
int spk_op_conv_group_dgrad(const void* dy_dev, const float* w_dev, void* dx_dev, int accumulate, int n, int h, int w,
                            int c, int groups, int stride, void* hip_stream);
int spk_op_conv_group_wgrad(const void* x_dev, const void* dy_dev, float* dw_dev, int n, int h, int w, int c, int groups,
                            int stride, void* hip_stream);
/* fp8 pointwise conv (the 1x1 convs of the fp8 EfficientNet mode): y = act((e4m3(A) . e4m3(W)^T) * factor + bias)
 * (+ res).  x: [m_rows][cin] fp16 (a_fp8 = 0: converted as x / a_scale) or e4m3 bytes (a_fp8 = 1: value = byte *
 * a_scale; gate, optional: fp32 [m_rows / hw][cin] multiplied in and re-rounded); w: float32 [cout][cin];
 * y: [m_rows][cout] fp16 or e4m3 bytes (out_fp8: byte = e4m3(value / y_scale)); bn_scale / bn_bias: float[cout]. */
int spk_op_pw_fp8(const void* x_dev, int a_fp8, const float* w_dev, void* y_dev, int out_fp8, const void* res_dev,
                  const float* bn_scale_dev, const float* bn_bias_dev, const float* gate_dev, int hw, int m_rows, int cin,
                  int cout, int act, float a_scale, float y_scale, void* hip_stream);
/* Eval-path 1x1 convolution (Conv2d(k=1, bias=False) + eval BatchNorm2d (+ shortcut) (+ ReLU); the 36 pointwise convs
 * `net(x)` runs in a ResNet-50 forward, sykepic/compute/probability.py:189).  x [n,h,w,cin] fp16 NHWC, w float32
 * [cout][cin], bn_scale / bn_bias float[cout] (folded statistics), res (optional) and y [n,ho,wo,cout] fp16;
 * stride 1 or 2; relu 0 / 1; split != 0: weights as fp16 hi + lo.  cfg >= 0: that tile configuration of the
 * direct-operand kernel (0 .. spk_op_conv1x1_num_configs() - 1; SPK_ERR_UNSUPPORTED when it does not fit the
 * problem), cfg < 0: the implicit-GEMM kernel.  Channel counts: multiples of 64.  Synchronous. */
int spk_op_conv1x1(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                   const void* res_dev, void* y_dev, int n, int h, int w, int cin, int cout, int stride, int relu,
                   int split, int cfg, void* hip_stream);
int spk_op_conv1x1_num_configs(void);
/* Eval-path 3x3 stride-1 pad-1 convolution (Conv2d(k=3, padding=1, bias=False) + eval BatchNorm2d (+ ReLU): the
 * middle conv of the bottleneck blocks `net(x)` runs, sykepic/compute/probability.py:189).  x [n,h,w,cin] fp16 NHWC,
 * w float32 [cout][3][3][cin], y [n,h,w,cout] fp16.  cfg >= 0: that tile configuration of the LDS-window kernel
 * (conv_c3.hip; SPK_ERR_UNSUPPORTED when it does not fit), cfg < 0: the implicit-GEMM kernel.  res_dev (may be null):
 * shortcut [n,h,w,cout] fp16 added before the activation (the block-closing conv of a ResNet-18/34 basic block).
 * Synchronous. */
int spk_op_conv3x3(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                   const void* res_dev, void* y_dev, int n, int h, int w, int cin, int cout, int relu, int split, int cfg,
                   void* hip_stream);
int spk_op_conv3x3_num_configs(void);
/* The direct 3x3 kernel of the 64 -> 64 channel convs (csrc/conv_d3.hip: weights resident in LDS, activation fragments
 * loaded straight into registers) on caller-provided DEVICE buffers: x [n,h,w,cin] fp16, w [cout][3][3][cin] fp32, pad 1.
 * cfg >= 0: that configuration - SPK_ERR_UNSUPPORTED ("does not fit") unless cin = cout = 64, stride 1 and split == 0;
 * cfg < 0: the implicit-GEMM kernel on the same problem (bit-identical where both run).  iters > 0 with ms_out: the
 * launch is repeated iters times and *ms_out is the mean time of one in milliseconds. */
int spk_op_conv3x3_direct(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                          const void* res_dev, void* y_dev, int n, int h, int w, int cin, int cout, int stride, int relu,
                          int split, int cfg, int iters, float* ms_out, void* stream);
int spk_op_conv3x3_direct_num_configs(void);
/* A whole identity bottleneck block of the eval path (torchvision Bottleneck.forward without downsample, reached through
 * `net(x)`: /root/reference/sykepic/compute/probability.py:189): y = ReLU(BN3(W3 . ReLU(BN2(W2 * ReLU(BN1(W1 . x))))) + x).
 * x, y: [n,h,w,4 cm] fp16 device tensors (y != x); fp32 device weights w1 [cm][4 cm], w2 [cm][3][3][cm], w3 [4 cm][cm];
 * folded eval-BatchNorm scale / shift vectors.  fused != 0: one kernel (csrc/conv_bneck.hip), SPK_ERR_UNSUPPORTED when
 * the shape has no instantiation; fused == 0: the three launches of the eval path.  iters > 0: *ms_out = mean time of one
 * block over `iters` repetitions. */
int spk_op_bottleneck(const void* x_dev, const float* w1_dev, const float* w2_dev, const float* w3_dev, const float* s1_dev,
                      const float* b1_dev, const float* s2_dev, const float* b2_dev, const float* s3_dev, const float* b3_dev,
                      void* y_dev, int n, int h, int w, int cm, int fused, int iters, float* ms_out, void* stream,
                      unsigned long long* stamps_dev /* diagnostics: [blocks][8] shader-clock stamps of the fused kernel, or null */,
                      /* optional: the 1x1 conv + BatchNorm + ReLU that reads the block's output (the next block's conv1):
                       * wz [coutz][4 cm] fp32, z [n,h,w,coutz] fp16.  fused == 2: conv1 on its own, then conv2 + conv3 + shortcut
                       * (+ that conv) as one kernel (conv_btail_kernel) */
                      const float* wz_dev, const float* sz_dev, const float* bz_dev, void* z_dev, int coutz);
/* Two chained 1x1 convs in ONE launch (round 4, csrc/conv_pw.hip): y = act(BN(W . x) + res) with cout = 256, then
 * z = actz(BNz(Wz . y)) computed from the output tile while it is still in registers - what the eval path runs for a
 * bottleneck's block-closing conv and the next block's first conv in the single-weight-image modes (the trunk y is
 * written for later shortcut adds, but never re-read by the conv that follows).  Tensors NHWC fp16 on the device,
 * weights fp32 [cout][cin] / [coutz][cout].  y and z are bit-identical to two spk_op_conv1x1(split = 0) calls. */
int spk_op_conv1x1_chain(const void* x, const float* w, const float* bn_scale, const float* bn_bias, const void* res,
                         void* y, const float* wz, const float* bnz_scale, const float* bnz_bias, void* z, int n, int h,
                         int wd, int cin, int cout, int coutz, int relu, int reluz, void* stream);
/* A block-closing 1x1 conv and the block's 1x1 shortcut (downsample) conv as ONE K-concatenated GEMM (round 3,
 * csrc/conv_pw.hip / conv_pwr.hip, PwConvArgs::x2): y = act(BN1(W1 . x) + BN2(W2 . x2[stride2])) - what the eval path
 * runs in the first block of every ResNet stage (torchvision Bottleneck.forward with `downsample`, reached through
 * `net(x)`: sykepic/compute/probability.py:189).  x [n,ho,wo,cin], x2 [n,h2,w2,cin2], y [n,ho,wo,cout] NHWC fp16 on the
 * device; weights fp32 [cout][cin] / [cout][cin2]; s / b: the folded eval-BatchNorm scale and shift of each conv.
 * cfg: a configuration of the 1x1 kernels, 0 .. spk_op_conv1x1_num_configs() - 1 (SPK_ERR_UNSUPPORTED when it does not
 * fit the problem); every configuration gives the same bits. */
int spk_op_conv1x1_dual(const void* x, const float* w1, const float* s1, const float* b1, const void* x2, const float* w2,
                        const float* s2, const float* b2, void* y, int n, int ho, int wo, int cin, int h2, int w2d, int cin2,
                        int cout, int stride2, int relu, int split, int cfg, void* stream);
/* Zero-sum rounding (csrc/zero_sum.hip) of fp32 weight rows on caller-provided DEVICE buffers: w, out [rows][row_len],
 * mu [mu_period] (element k weighted with mu[k % mu_period]) or NULL (all ones).  out[i] is fp16(w[i]) or the fp16
 * neighbour on the other side of w[i]; per row sum_k mu_k (out_k - w_k) is driven to ~0.  Synchronises the stream. */
int spk_op_zero_sum_round(const float* w_dev, const float* mu_dev, float* out_dev, int64_t rows, int row_len,
                          int mu_period, void* stream);
/* Depthwise Conv2d(C, C, k, stride, pad (k-1)/2, groups=C) + folded BatchNorm + activation act (SPK_ACT_*; MBConv):
 * x [n,h,w,C] fp16 NHWC, w float32 [C][k*k], y [n,ho,wo,C] fp16; pool (optional) float32 [n][C] = per-image sums of
 * the outputs (squeeze-excitation numerator).  lds != 0: the LDS row-ring kernel, else the gather kernel. */
int spk_op_dwconv(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev, void* y_dev,
                  float* pool_dev, int n, int h, int w, int channels, int k, int stride, int act, int lds, void* hip_stream);

/* --- Test hooks: single operators of the MBConv training step (csrc/train_effnet.hip) ---
 * What `out = net(x)` (train mode) and `loss.backward()` run for ONE layer of an EfficientNet-B0...B7 / MobileNetV3
 * (sykepic/train/train.py:240,242): the launches spk_train_forward_backward makes for it, chosen by the functions the
 * step itself calls.  Layout as in the step: activations and gradients bf16 NHWC device buffers of C channels, C the
 * padded channel count (a multiple of 64); c_log <= C the layer's own count, pad channels hold zeros; parameters and
 * their gradients float32, c_log entries.  A NULL output pointer skips that part.  Synchronous.
 *
 * Depthwise Conv2d(c_log, c_log, k, stride, pad, groups = c_log), k 3 or 5, stride 1 or 2: x [n,h,w,C], dy [n,ho,wo,C],
 * w float32 [c_log][k*k] (packed inside the call to the tap-major window and its flipped copy, bf16-rounded, as the step
 * packs it).  y: the raw output [n,ho,wo,C]; dx [n,h,w,C] (= or, accumulate != 0, +=) the data gradient; dw float32
 * [c_log][k*k].  The kernels are the step's: pad (k-1)/2 runs the eval path's kernel in bf16 (forward; stride-1 dx that is
 * not accumulated, on the flipped window) and dw_dgrad_px_kernel, any other pad dw_fwd_kernel / dw_dgrad_kernel. */
int spk_op_dw_train(const void* x_dev, const void* dy_dev, const float* w_dev, void* y_dev, void* dx_dev, float* dw_dev,
                    int accumulate, int n, int h, int w, int channels, int c_log, int k, int stride, int pad,
                    void* hip_stream);
/* BatchNorm2d (train mode) + activation (SPK_ACT_*) forward on raw [n*hw][C]: column sums -> finalize -> apply.
 * out = act(raw * scale + shift) * rowscale[image] + res; res (bf16 [n*hw][C]) and rowscale (float32 [n], the stochastic
 * depth factor) are optional.  pool_part != NULL (float32 [n][chunks][C], chunks = 1 / 4 / 16 for hw < 196 / < 3136 /
 * more; res and rowscale must be NULL): the form that also leaves the per-chunk channel sums of `out` for the
 * squeeze-excitation layer behind.  st: float32 [4][C] = batch mean, invstd, scale, shift (zeros in the pad channels);
 * running_mean / running_var [c_log] are updated in place (unbiased variance). */
int spk_op_bna_forward(const void* raw_dev, const float* gamma_dev, const float* beta_dev, float* running_mean_dev,
                       float* running_var_dev, const void* res_dev, const float* rowscale_dev, void* out_dev,
                       float* pool_part_dev, float* st_dev, int n, int hw, int channels, int c_log, int act, float eps,
                       float momentum, void* hip_stream);
/* Its backward: g = gradient of `out`, st as spk_op_bna_forward left it.  dy [n*hw][C] = gradient of raw, dgamma /
 * dbeta [c_log] (either may be NULL), g_res (optional) receives (or, res_accumulate != 0, adds) the shortcut's gradient. */
int spk_op_bna_backward(const void* g_dev, const void* raw_dev, const float* st_dev, const float* gamma_dev,
                        const float* rowscale_dev, void* dy_dev, float* dgamma_dev, float* dbeta_dev, void* g_res_dev,
                        int res_accumulate, int n, int hw, int channels, int c_log, int act, void* hip_stream);
/* Squeeze-excitation forward: out = a * gate, gate = sigmoid(W2 silu(W1 mean_hw(a) + b1) + b2) (gate_kind 1: Hardsigmoid /
 * ReLU).  a, out [n][hw][C]; W1 [S][c_log], b1 [S], W2 [c_log][S], b2 [c_log], S <= 256 (else SPK_ERR_UNSUPPORTED).
 * Saved for the backward pass, float32: pooled [n][C], u1 [n][S] (W1 pooled + b1), h1 [n][S], gate [n][C].
 * pool_part (optional): the channel sums spk_op_bna_forward left, used instead of pooling `a`; out == NULL: gates only. */
int spk_op_se_train_forward(const void* a_dev, const float* pool_part_dev, const float* w1_dev, const float* b1_dev,
                            const float* w2_dev, const float* b2_dev, float* pooled_dev, float* u1_dev, float* h1_dev,
                            float* gate_dev, void* out_dev, int n, int hw, int channels, int c_log, int s_hidden,
                            int gate_kind, void* hip_stream);
/* Its backward: da [n][hw][C] from g (gradient of out), a and the saved vectors; gW1 [S][c_log], gb1 [S], gW2 [c_log][S],
 * gb2 [c_log] (each optional).  du2 [n][C] / du1 [n][S] receive the gradients of the two pre-activations; pool_part
 * (optional) the per-chunk sums over hw of g * a.  g == NULL: only the parameter-gradient kernel, on the caller's du2 /
 * du1 / h1 / pooled. */
int spk_op_se_train_backward(const void* g_dev, const void* a_dev, const float* gate_dev, const float* u1_dev,
                             const float* h1_dev, const float* pooled_dev, const float* w1_dev, const float* w2_dev,
                             float* du2_dev, float* du1_dev, float* pool_part_dev, void* da_dev, float* gw1_dev,
                             float* gb1_dev, float* gw2_dev, float* gb2_dev, int n, int hw, int channels, int c_log,
                             int s_hidden, int gate_kind, void* hip_stream);
/* The 3x3 stride-2 pad-1 stem: x [n][h][w rounded up to even][4] bf16 holding pixel values x 255 (zeros in the unused
 * channels and the pad column), w float32 [cout][9][cin], cin <= 4, cout <= 85.  y: raw output [n,ho,wo,C] (NULL: skipped);
 * dw float32 [cout][9][cin] from dy [n,ho,wo,C] (NULL: skipped), scaled by 1 / 255 as in the step. */
int spk_op_stem3_train(const void* x_dev, const float* w_dev, const void* dy_dev, void* y_dev, float* dw_dev, int n, int h,
                       int w, int cin, int cout, int channels, void* hip_stream);
/* Launch geometry those kernels would get (host arithmetic only, no GPU needed; the launchers' own helpers):
 *   kind 0 (col_stats / bna_*: m rows, C) and kind 1 (depthwise weight gradient: m = n * ho * ceil(wo / 4) items, C):
 *     out = rows per block, blocks, channel tiles, channels per tile, rows in flight, idle threads of 256,
 *           8-channel groups of the last tile
 *   kind 2 (pool_partial / bna_apply_pool: hw, C): the same with rows per block = rows of a chunk, blocks = chunks
 *   kind 3 (squeeze-excitation gates: m = c_log, s hidden units): out = rows of W2 per tile, gate tiles, hidden units per
 *     lane of se_bwd1 (NQ), hidden units per thread of se_wgrad (SJ), blocks of se_wgrad; s > 256: SPK_ERR_UNSUPPORTED
 *   kind 4 (depthwise: m = k, C = stride, hw = pad, s = accumulate): out = forward form, data-gradient form;
 *     0 the eval path's LDS-window kernel, 1 dw_dgrad_px_kernel, 2 the gather kernels, -1 none */
int spk_op_mbconv_geometry(int kind, int m, int channels, int hw, int s_hidden, int out[8]);

/* --- Test hooks: single operators of the MBConv EVAL path and the eval stems ---
 * (csrc/conv_igemm.hip PADC / GATE, csrc/effnet.hip, csrc/conv_stem.hip): the pack and launch calls the model executor
 * makes for ONE such layer, through its own dispatch functions.  Every pointer is device memory, activations are fp16
 * NHWC with exactly the stated channel count stored, parameters float32.  Synchronous.
 *
 * 1x1 conv + folded BatchNorm (+ shortcut) + activation on tensors whose channel counts are multiples of 8 only: the
 * GEMM is padded to multiples of 64 inside (spk_launch_pack_padded, ConvArgs::cin_s / cout_s).  x [n,h,w,cin], w
 * [cout][cin], res (optional) and y [n,h,w,cout].  gate (optional) float32 [n][cin]: the activation operand is
 * fp16(x * gate), the squeeze-excitation scaling multiplied in where the conv stages its operand (spk_set_gate).
 * act: SPK_ACT_*.  Honours spk_op_conv_pin; SPK_ERR_UNSUPPORTED ("does not fit") for a pinned flavour the padded or gated
 * path does not instantiate. */
int spk_op_conv1x1_padded(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                          const void* res_dev, const float* gate_dev, void* y_dev, int n, int h, int w, int cin, int cout,
                          int act, int split, void* hip_stream);
/* Squeeze-excitation of the eval path from the caller's pool partials [n][chunks][c] (sums over hw, as the depthwise
 * kernels leave them): hid [n][sq] = act1(W1 . mean + b1), scale [n][c] = act2(W2 . hid + b2), y = x * scale (y NULL:
 * the gates only).  w1 [sq][c], w2 [c][sq] (transposed inside, as spk_commit does).  gate_kind 0: SiLU, Sigmoid; 1: ReLU,
 * Hardsigmoid.  The kernels keep hid directly behind the gates: hid_out must be scale_out + n * c (one buffer). */
int spk_op_se_eval(const void* x_dev, const float* partial_dev, int chunks, const float* w1_dev, const float* b1_dev,
                   const float* w2_dev, const float* b2_dev, float* hid_out_dev, float* scale_out_dev, void* y_dev, int n,
                   int hw, int channels, int squeeze, int gate_kind, void* hip_stream);
/* The 3x3 stride-2 pad-1 RGB stem of the eval path: x [n][h][w rounded up to even][4] fp16 holding pixel values x 255
 * (zeros in channel 3 and the pad column), w [cout][3][3][3], y [n,ho,wo,cout]; 1 / 255 is folded into the epilogue
 * scale as spk_commit does.  cout a multiple of 8, at most 256. */
int spk_op_stem3_eval(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                      void* y_dev, int n, int h, int w, int cout, int act, void* hip_stream);
/* The 7x7 stride-2 pad-3 stem (3 -> 64, ReLU) of the eval path on the same input layout, w [64][7][7][3], split: hi +
 * lo fp16 weight images.  pool_y NULL: y [n,ho,wo,64].  pool_y set: the kernel variant that also applies the 3x3
 * stride-2 pad-1 max-pool and writes ONLY pool_y [n,(ho-1)/2+1,(wo-1)/2+1,64] (y is not touched and may be NULL). */
int spk_op_stem7_eval(const void* x_dev, const float* w_dev, const float* bn_scale_dev, const float* bn_bias_dev,
                      void* y_dev, void* pool_y_dev, int n, int h, int w, int split, void* hip_stream);
/* What the launchers of those kernels choose (host arithmetic only, no GPU needed; the launchers' own helpers):
 *   kind 0 (squeeze-excitation gates: a = n, b = chunks, c = channels, d = hidden units): out = CH instantiation of
 *     se_fc1 (0: the run-time loop), clamped surplus loads of the run-time loop's last step, images of the last block,
 *     hidden units the last fc1 block leaves out, staging passes of se_fc2, channel tiles of se_fc2, channels of the last
 *     tile, image blocks
 *   kind 1 (se_scale: a = n, b = hw, c = channels): out = grid x, blocks that would cover one image once
 *   kind 2 (3x3 stem: a = ho, b = wo, c = cout): out = GT instantiation (0: run-time divisions)
 *   kind 3 (padded / gated 1x1 conv: a = tile config, b = main-loop flavour, c = GEMM couts, d = split + 2 x gated):
 *     out = narrowed tile config, DMA template argument of the instantiation or -3 when there is none */
int spk_op_mbconv_eval_geometry(int kind, int a, int b, int c, int d, int out[8]);

/* --- Test hooks: single operators of the classifier head, the loss and the pooling layers ---
 * (csrc/head.hip, csrc/pointwise.hip, csrc/train_kernels.hip): the launches `net(x)`, `criterion(out, y)` and
 * `loss.backward()` (sykepic/train/train.py:240-242, sykepic/compute/probability.py:189-194) reach for ONE such layer,
 * through the launcher functions the model executor and the training step call.  Every pointer is device memory;
 * head tensors are float32 row-major, pooling tensors NHWC with c a multiple of 8.  Synchronous.
 *
 * y [n][out] = x [n][in] . w [out][in]^T + b [out] (b may be NULL): the MFMA kernel when in % 4 == 0, else the GEMM. */
int spk_op_linear(const float* x_dev, const float* w_dev, const float* b_dev, float* y_dev, int n, int in, int out,
                  void* hip_stream);
/* Its backward as the training step runs it: dw [out][in] = gy^T . x, db [out] = column sums of gy, dx [n][in] = gy . w;
 * a NULL output is skipped (x is needed for dw only, w for dx only).  form: -1 the GEMM kernel the step uses
 * (SPK_SGEMM_FMA), 0 the MFMA kernel, 1 the LDS-tiled FMA kernel. */
int spk_op_linear_backward(const float* gy_dev, const float* x_dev, const float* w_dev, float* dw_dev, float* db_dev,
                           float* dx_dev, int n, int in, int out, int form, void* hip_stream);
/* p [n][c] = softmax(z * logf(base)) per row (the base-1.3 softmax of net_pass is base = 1.3). */
int spk_op_softmax(const float* z_dev, float* p_dev, int n, int c, float base, void* hip_stream);
/* CrossEntropyLoss(reduction mean) and its gradient: stats[0] += sum of the row losses, stats[1] += rows whose arg-max
 * (lowest index among the maxima) is the label; dz [n][c] (may be NULL) = (softmax(z) - onehot) / n.  labels: int64 [n],
 * each in [0, c). */
int spk_op_cross_entropy(const float* z_dev, const int64_t* labels_dev, int n, int c, float* stats_dev, float* dz_dev,
                         void* hip_stream);
/* CrossEntropyLoss(weight = w, label_smoothing, reduction mean), the kernel spk_model_set_loss switches the steps to:
 * stats[0] += n * loss, stats[1] as above; dz [n][c] (may be NULL) = d loss / d z; w_dev float32 [c] of positive weights
 * or NULL (all ones); counts_dev int32 [c][2] (may be NULL) += per class (rows seen, rows correct).  label_smoothing
 * outside [0, 1]: SPK_ERR_ARG.  Equal inputs give equal bits. */
int spk_op_cross_entropy_ex(const float* z_dev, const int64_t* labels_dev, int n, int c, const float* w_dev,
                            float label_smoothing, float* stats_dev, int* counts_dev, float* dz_dev, void* hip_stream);
/* The Mixup / CutMix criterion of that loss on two label vectors, the kernel spk_train_forward_backward_pair runs:
 * L = lam CE(z, ya; w, eps) + (1 - lam) CE(z, yb; w, eps), each CE normalised by its own sum of weights, 1 - lam formed
 * in float32.  stats[0] += n * L; dz [n][c] (may be NULL) = lam dCE_a/dz + (1 - lam) dCE_b/dz; stats[1] and counts_dev
 * (may be NULL) count against the dominant label: ya when lam >= 0.5, else yb.  yb_dev == NULL or lam == 1: the bits of
 * spk_op_cross_entropy_ex on ya.  lam or label_smoothing outside [0, 1] or not finite: SPK_ERR_ARG.  Equal inputs give
 * equal bits. */
int spk_op_cross_entropy_pair(const float* z_dev, const int64_t* ya_dev, const int64_t* yb_dev, float lam, int n, int c,
                              const float* w_dev, float label_smoothing, float* stats_dev, int* counts_dev, float* dz_dev,
                              void* hip_stream);
/* That criterion distilled against a teacher's logits t_dev [n][c], the kernel spk_train_forward_backward_distill runs:
 * L = (1 - alpha) L_hard + alpha KD, KD = T^2 / n sum_i KL(softmax(t_i / T) || softmax(z_i / T)), L_hard the loss of
 * spk_op_cross_entropy_pair (yb_dev == NULL or lam == 1: of spk_op_cross_entropy_ex on ya), 1 - alpha formed in float32.
 * stats[0] += n * L; stats[1] and counts_dev as there; dz [n][c] (may be NULL) = (1 - alpha) dL_hard/dz + (alpha T / n)
 * (softmax(z / T) - softmax(t / T)); kd_stats_dev float32 [2] (may be NULL): [0] += n * KD, [1] += rows whose arg-max
 * of z equals that of t (lowest index among the maxima).  t_dev == NULL or alpha == 0: the bits of
 * spk_op_cross_entropy_pair, t_dev not read, kd_stats_dev not written.  lam, label_smoothing or alpha outside [0, 1],
 * temperature not finite or <= 0, kd_stats_dev without t_dev: SPK_ERR_ARG.  Equal inputs give equal bits. */
int spk_op_cross_entropy_distill(const float* z_dev, const int64_t* ya_dev, const int64_t* yb_dev, float lam,
                                 const float* t_dev, float alpha, float temperature, int n, int c, const float* w_dev,
                                 float label_smoothing, float* stats_dev, int* counts_dev, float* kd_stats_dev,
                                 float* dz_dev, void* hip_stream);
/* MaxPool2d(k, stride, pad): x [n,h,w,c] -> y [n,ho,wo,c].  idx == NULL: the eval path's kernel, dtype 0 bf16 / 1 fp16.
 * idx [n,ho,wo,c] bytes: the training step's kernel (bf16 only), which also saves the tap r * k + s of each maximum (the
 * first in that order among equal values).  c % 8 != 0: SPK_ERR_ARG; k * k > 255 or pad > k / 2: SPK_ERR_UNSUPPORTED. */
int spk_op_maxpool(const void* x_dev, void* y_dev, unsigned char* idx_dev, int n, int h, int w, int c, int k, int stride,
                   int pad, int dtype, void* hip_stream);
/* Its backward: gx [n,h,w,c] bf16 = for each pixel the sum of gy over the windows whose saved tap points at it.
 * form: -1 the kernel the step uses (SPK_POOL_PAIR), 0 the per-pixel kernel (compiled for k3 s2 p1, run-time k / stride /
 * pad otherwise), 1 the pixel-pair kernel (k3 s2 p1 and an even width, else SPK_ERR_UNSUPPORTED). */
int spk_op_maxpool_backward(const void* gy_dev, const unsigned char* idx_dev, void* gx_dev, int n, int h, int w, int c,
                            int k, int stride, int pad, int form, void* hip_stream);
/* AdaptiveAvgPool2d(1): x [n][hw][c] (dtype 0 bf16 / 1 fp16) -> y float32 [n][c]; backward gx [n][hw][c] bf16 = gy / hw. */
int spk_op_gavgpool(const void* x_dev, float* y_dev, int n, int hw, int c, int dtype, void* hip_stream);
int spk_op_gavgpool_backward(const float* gy_dev, void* gx_dev, int n, int hw, int c, void* hip_stream);

/* --- ROI preprocessing straight from the .roi blob ---
 * One ROI of an IFCB sample: byte offset into the .roi blob, width, height
 * (columns 17/15/16 of the .adc line, sykepic/utils/ifcb.py:100-110). */
typedef struct {
  int64_t offset;
  int32_t width, height;
} spk_roi;
/* blob -> [n, out_h, out_w, 3] uint8 (mode/black/white border, aspect-preserving
 * OpenCV-style fixed-point bilinear resize), replacing the PNG round trip +
 * ImageDataset + Compose of the reference (sykepic/utils/ifcb.py:76-118,
 * sykepic/train/data.py:210-231, sykepic/train/image.py:25-56).  border: -1 =
 * the ROI's modal grey level, else a grey value 0..255.  The result feeds
 * spk_forward_infer(layout NHWC, dtype U8).  All pointers are device memory. */
int spk_preprocess_rois(const unsigned char* blob_dev, int64_t blob_bytes, const spk_roi* rois_dev,
                        int n, int out_h, int out_w, int border, unsigned char* out_dev, void* hip_stream);

/* Training augmentations on a batch of resized+bordered uint8 NHWC images:
 * replaces the cv2 calls of sykepic/train/image.py:80-180 that Compose.__call__ (image.py:25-56) makes per
 * image in the DataLoader workers.  The random draws stay on the host (Python `random`, reference call order);
 * ops_dev is [n_ops][n]: op j of every sample, applied in order, each rounding to uint8 as the host does.
 *   FLIP_H / FLIP_V: i0 = apply flag            TRANSLATE: i0 = x shift, i1 = y shift (constant border)
 *   ZOOM: d[0] = zoom factor f, i0 = side of the resized square (cvRound(w * f)); cv2.resize(fx = fy = f), then
 *         centred pad (f < 1) or crop
 *   ROTATE: d[0..5] = the 2x3 matrix as cv::warpAffine inverts it (row major); OpenCV's fixed-point bilinear
 *           warp (1/32-pixel coordinates, 15-bit weight table), constant border
 *   BRIGHT: d[0] = factor, truncating
 * border_dev: [n][4] bytes (one value per channel).  tmp_dev: scratch of the batch size (needed when n_ops > 1).
 * The result is written to out_dev. */
#define SPK_AUG_FLIP_H 1
#define SPK_AUG_FLIP_V 2
#define SPK_AUG_TRANSLATE 3
#define SPK_AUG_ZOOM 4
#define SPK_AUG_ROTATE 5
#define SPK_AUG_BRIGHT 6
typedef struct {
  int32_t kind;
  int32_t i0, i1;
  int32_t pad_;
  double d[6];
} spk_aug_op;
int spk_augment_batch(const unsigned char* in_dev, unsigned char* out_dev, unsigned char* tmp_dev, int n, int h,
                      int w, int c, const spk_aug_op* ops_dev, int n_ops, const unsigned char* border_dev,
                      void* stream);

/* Mixup / CutMix (not in the reference; torchvision's reference recipe): every image of a batch mixed with the image
 * `shift` places before it, out[i] = in[i] outside the box [y1,y2) x [x1,x2) and ca * in[i] + cb * in[(i - shift) mod n]
 * inside it; one box and one coefficient pair for the batch.  Mixup is the full-image box with (ca, cb) =
 * (lam, 1 - lam); CutMix is (0, 1), which copies the partner's elements bit for bit, without arithmetic.  Each product
 * is rounded to float32, then the sum; float32 batches store that value, uint8 batches store it rounded to the nearest
 * integer (ties to even) and clamped to 0..255.  Batches: SPK_LAYOUT_NHWC / SPK_DTYPE_U8 [n,h,w,c] or SPK_LAYOUT_NCHW /
 * SPK_DTYPE_F32 [n,c,h,w], c 1 or 3, any n, h, w >= 1 and any pointer alignment the element type allows.  Out of
 * place: in_dev and out_dev must not overlap.  An empty box is a plain copy.  Checked before any HIP call, each
 * SPK_ERR_ARG: a null pointer, n / h / w < 1, c not 1 or 3, another layout / dtype pair, shift outside [0, n), ca or cb
 * not finite, a box outside the image or inverted, overlapping buffers.  Asynchronous on hip_stream. */
int spk_mix_batch(const void* in_dev, void* out_dev, int n, int h, int w, int c, int layout, int dtype,
                  int shift, float ca, float cb, int y1, int x1, int y2, int x2, void* hip_stream);

/* Test-time augmentation (not in the reference, which classifies every ROI once): the symmetric views of a batch and
 * the mean of the probabilities they give.  A view code v is in 0..7, the dihedral group of the square: bit value 4
 * transposes H and W and is applied first, bit value 2 then reverses the rows, bit value 1 the columns - 0 identity,
 * 1 / 2 the flips, 3 the half turn, 4 the transpose, 5 / 6 the quarter turns, 7 the anti-transpose.
 * spk_tta_views: out_dev = [k][n] images, view-major, out[j * n + i] = T_views[j](in[i]); every output element is a
 * copy of one input element, bit for bit (no arithmetic), one launch writes all k views and reads each input tile
 * once.  Batches as for spk_mix_batch: SPK_LAYOUT_NHWC / SPK_DTYPE_U8 [n,h,w,c] or SPK_LAYOUT_NCHW / SPK_DTYPE_F32
 * [n,c,h,w], c 1 or 3, any n, h, w >= 1 and any pointer alignment the element type allows.  views_host: k codes in
 * host memory, duplicates allowed.  Out of place.  Checked before any HIP call, each SPK_ERR_ARG: a null pointer,
 * n / h / w < 1, c not 1 or 3, another layout / dtype pair, k outside 1..8, a code outside 0..7, a transposing code
 * with h != w, overlapping buffers.  Asynchronous on hip_stream. */
int spk_tta_views(const void* in_dev, void* out_dev, int n, int h, int w, int c, int layout, int dtype,
                  const int32_t* views_host, int k, void* hip_stream);
/* p_dev = [k][numel], out_dev = [numel]: out[j] = ((...(p[0][j] + p[1][j]) + ...) + p[k-1][j]) / (float)k - float32
 * adds in view order, then one IEEE float32 division (no reciprocal multiply, no contraction): a defined bit pattern.
 * k in 1..8, numel >= 1, any 4-byte alignment.  Checked before any HIP call, each SPK_ERR_ARG: a null pointer, k
 * outside 1..8, numel < 1, overlapping buffers.  Asynchronous on hip_stream. */
int spk_tta_mean(const float* p_dev, float* out_dev, int k, int64_t numel, void* hip_stream);

/* --- prediction from probabilities and thresholds ---
 * row_prediction of sykepic/compute/prediction.py:49-71 for n rows at once:
 * thresholds_dev = float[num_classes] (+inf for a class without a threshold):
 * the highest-probability class with p >= its own threshold, classified = 1;
 * if none, arg-max with classified = 0.  thresholds_dev == NULL: arg-max and
 * classified = p > scalar_threshold.  pred_dev int32[n], classified_dev u8[n]. */
int spk_predict_rows(const float* probs_dev, int n, int num_classes, const float* thresholds_dev,
                     float scalar_threshold, int32_t* pred_dev, unsigned char* classified_dev,
                     void* hip_stream);

/* Per-layer timing of the last spk_forward_infer call (HIP events on the
 * model's stream); used by bench.py for the roofline line. Returns the
 * number of records written. */
typedef struct {
  char name[96];
  float ms;
  double flops;
  double bytes;
} spk_layer_time;
int spk_model_profile_infer(spk_model* m, const void* x_dev, int n, int h, int w, int layout,
                            int dtype, int iters, spk_layer_time* out, int cap);

/* Per-phase timing of spk_train_forward_backward (same event method): one
 * record per kernel group (conv fwd / dgrad / wgrad, BN, pooling, head...);
 * `flops` = algorithmic FLOPs of the phase, `bytes` = launches per step. */
int spk_model_profile_train(spk_model* m, const void* x_dev, int n, int h, int w, int layout,
                            int dtype, const int64_t* y_dev, float* stats_dev, int iters,
                            spk_layer_time* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
