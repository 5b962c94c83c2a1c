/*
 * include/nrc_hpm.h -- C ABI of the MI355X-native NRC-HPM hot path (libnrc_hpm.so).
 *
 * Drop-in boundary for the reference's hot path.  Each entry point cites the
 * reference interface it replaces (paths relative to the reference checkout).  Plain pointers and sizes only;
 * `stream` arguments are hipStream_t passed as void* (0 = the null stream).  All functions return NRC_OK (0) or
 * a negative error code and never abort; nrc_last_error() gives the thread-local message (the reference throws
 * std::runtime_error("SkyRenderer ERROR: ..."), src/Log.cpp:16-20 -- the C++ layer in nrc_hpm.hpp does the same).
 *
 * Vulkan/CUDA-interop types of the reference are replaced as follows:
 *   VkQueue                         -> hipStream_t (stream order replaces both external semaphores)
 *   cudaExternalSemaphore_t x2      -> dropped
 *   VkImage / VkImageView           -> device pointer to an RGBA32F row-major framebuffer
 */
#ifndef NRC_HPM_H
#define NRC_HPM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NRC_OK 0
#define NRC_ERR_INVALID (-1)    /* bad argument / unsupported configuration */
#define NRC_ERR_HIP (-2)        /* a HIP runtime call failed (message holds hipGetErrorString) */
#define NRC_ERR_STATE (-3)      /* call order violated (e.g. InferAndTrain before Init) */
#define NRC_ERR_COMM (-4)       /* multi-GPU: a collective failed or a peer did not answer in time; the communicator is aborted (see
                                 * nrc_cache_comm_status) -- every later call that needs it fails at once, destroy the cache */

const char* nrc_last_error(void);
const char* nrc_version(void);

/* ---------------------------------------------------------------------------------------------------------
 * en::AppConfig (include/engine/AppConfig.hpp:9-66; 17 positional CLI args src/AppConfig.cpp:154-182,
 * defaults src/main.cu:429-440).  Scene preset values (src/AppConfig.cpp:93-150) are carried explicitly. */
/* The reference passes lossFn / optimizer through to tiny-cuda-nn unchecked (src/NeuralRadianceCache.cu:17-26); this build implements a
 * CLOSED set -- the seven losses and two optimizers named below -- and nrc_cache_create fails with NRC_ERR_INVALID and a message that lists
 * them for any other tiny-cuda-nn name (Novograd, Shampoo, ...: update rules that could not be restated without the absent submodule;
 * CrossEntropy, Variance: they need a sample pdf the NRC path does not have). */
typedef struct nrc_config {
    char loss_fn[32];              /* "RelativeL2Luminance" | "L2" | "RelativeL2" | "L1" | "Mape" | "Smape" | "LogL1" (tiny-cuda-nn names) */
    char optimizer[32];            /* "Adam" (default) | "SGD": nested in the EMA wrapper, src/NeuralRadianceCache.cu:20-28 */
    float learning_rate;
    float ema_decay;
    uint32_t pos_id;               /* 0 HashGrid(16x2, 2^19) | 1 Identity | 2 TriangleWave-12 | 3 Frequency-12 */
    uint32_t dir_id;               /* 0 OneBlob-4 | 1 Identity | 2 TriangleWave-4 */
    uint32_t nn_width;             /* 64 (16, 32, 64, 128: tiny-cuda-nn's FullyFusedMLP widths) */
    uint32_t nn_depth;             /* n_hidden_layers, 6 */
    uint32_t log2_infer_batch_size;
    uint32_t log2_train_batch_size;
    uint32_t train_batch_count;
    uint32_t scene_id;
    float train_ring_buf_size;
    uint32_t train_spp;
    uint32_t primary_ray_length;
    float primary_ray_prob;
    uint32_t train_ray_length;
    /* additions of this build */
    uint32_t seed;                 /* weight-init seed (tiny-cuda-nn default 1337) */
    uint32_t compat_fix;           /* bit 0: fix quirk Q1 (TRAIN_Y_DIST), bit 1: fix quirk Q2 (trainRayLength); 0 = faithful */
    uint32_t hashgrid_log2_size;   /* posID 0: log2_hashmap_size; 0 = the reference's 19 (src/AppConfig.cpp:24) */
    uint32_t self_train;           /* NRC renderer only, read at creation: 0 (default) = the reference's training targets; 1 = self-training, below */
} nrc_config;
/* ABI note: self_train is new in nrc_version() "0.3" (the struct grew by 4 bytes); a caller built against an older header must be
 * recompiled (the library would read self_train past the end of its struct).
 *
 * Self-training (Mueller et al. 2021, "Real-time Neural Radiance Caching for Path Tracing"; the reference has none).  The train-path loop
 * (prep_train_rays.comp:80-95) runs L vertices per sample: L = 1 in the faithful mode (quirk Q2), L = train_ray_length with
 * NRC_FIX_Q2_TRAIN_RAY_LEN.  Sample s of train ray i ends with light_s (the sum it adds without self-training) and factor_s = 0.5^L when the
 * loop ran all L vertices without leaving the medium; the walk then stands at its last scatter point cur with the direction after its last
 * new_ray_dir, dir.  With self_train = 1:
 *   tail    only a sample that completed all L vertices has one: the query nrc_query(cur, dir), normalised as gen_rays' NRC query (quirk Q5,
 *           NaN phi, included).  A sample whose walk left the medium has no tail term (skipped, not multiplied by 0: 0 * Inf is NaN).
 *   weights the tail's radiance y_s is the cache's inference with the EMA weights that frame N's render inference reads -- those after
 *           frame N-1's last optimizer step (quirk Q13 ordering) -- for every train batch of the frame.
 *   target  per channel, fp32, no contraction, in this order: t_s = factor_s * fmaxf(0, y_s) (NaN -> 0); u_s = light_s + t_s;
 *           acc = ((0 + u_0) + u_1) + ...; target = fminf(8, acc / spp).  With y = 0 this is the target without self-training, bit for bit.
 * Training inputs, the ring buffer, the render path and compositing are unchanged; frames rendered with train = 0 infer no tails. */

#define NRC_FIX_Q1_TRAIN_Y_DIST 1u
#define NRC_FIX_Q2_TRAIN_RAY_LEN 2u

/* fills the defaults of src/main.cu:432-439, except for the position encoding: posID 3 (Frequency, the north-star model with
 * the fully fused kernels) instead of the reference's 0 (HashGrid) -- set pos_id = 0 for the reference's exact default */
void nrc_config_default(nrc_config* cfg);

/* ---------------------------------------------------------------------------------------------------------
 * en::NeuralRadianceCache (include/engine/graphics/NeuralRadianceCache.hpp:10-64, src/NeuralRadianceCache.cu) */
typedef struct nrc_cache nrc_cache_t;

/* NeuralRadianceCache::NeuralRadianceCache(const AppConfig&)  (src/NeuralRadianceCache.cu:11-40) */
int nrc_cache_create(const nrc_config* cfg, nrc_cache_t** out);
/* NeuralRadianceCache::Init(inferCount, dCuInferInput, dCuInferOutput, dCuTrainInput, dCuTrainTarget, sem, sem)
 * (src/NeuralRadianceCache.cu:42-95).  Buffers are caller-owned DEVICE memory: [n][5] / [n][3] fp32 AoS. */
int nrc_cache_init(nrc_cache_t* c, uint32_t infer_count, float* d_infer_input, float* d_infer_output,
                   float* d_train_input, float* d_train_target, void* stream);
/* The same Init with the reference's semaphore pair kept in HIP terms (include/engine/graphics/NeuralRadianceCache.hpp:15-22:
 * cudaExternalSemaphore_t cudaStartSemaphore, cudaFinishedSemaphore): start_event / finished_event are hipEvent_t of the caller
 * (either may be NULL).  Every InferAndTrain first makes its stream wait for start_event (AwaitCudaStartSemaphore,
 * src/NeuralRadianceCache.cu:158-167) and records finished_event behind its last kernel (SignalCudaFinishedSemaphore, :169-177). */
int nrc_cache_init_events(nrc_cache_t* c, uint32_t infer_count, float* d_infer_input, float* d_infer_output,
                          float* d_train_input, float* d_train_target, void* stream, void* start_event, void* finished_event);
/* NeuralRadianceCache::InferAndTrain(const uint32_t* inferFilter, bool train) (src/NeuralRadianceCache.cu:97-103).
 * infer_filter: HOST array, one entry per inference batch, >0 => run; NULL => run every batch. */
int nrc_cache_infer_and_train(nrc_cache_t* c, const uint32_t* infer_filter, int train);
/* NeuralRadianceCache::Destroy (src/NeuralRadianceCache.cu:105-107); frees the object */
int nrc_cache_destroy(nrc_cache_t* c);
/* GetLoss / Get{Infer,Train}Batch{Count,Size} (src/NeuralRadianceCache.cu:109-132).
 * The reference reads the loss back synchronously inside every training step (trainer->loss, :154) and GetLoss() returns that
 * value; its main loop polls it every frame (src/main.cu:303,376).  Here a one-thread kernel behind every training step stores
 * {loss, step number} into host-mapped pinned memory on the training stream:
 *   nrc_cache_get_loss        reference semantics: the loss of the last training step that was ENQUEUED (InferAndTrain / Render
 *                             with train, nrc_cache_backward); waits for that step only, not for the device.  0 before the first.
 *                             (nrc_cache_get_loss_blocking is the same call under its round-2 name.)
 *   nrc_cache_get_loss_async  never blocks and never drains the renderer's frame pipeline: *loss = the loss of the most recent
 *                             step that has COMPLETED, *step = that step's number (1-based; 0: none yet), *steps_enqueued = the
 *                             number of the newest step enqueued -- so a caller sees how stale the value is (at most the
 *                             pipeline depth, four frames).  step / steps_enqueued may be NULL. */
float nrc_cache_get_loss(nrc_cache_t* c);
float nrc_cache_get_loss_blocking(nrc_cache_t* c);
int nrc_cache_get_loss_async(nrc_cache_t* c, float* loss, uint32_t* step, uint32_t* steps_enqueued);
size_t nrc_cache_get_infer_batch_count(nrc_cache_t* c);
size_t nrc_cache_get_train_batch_count(nrc_cache_t* c);
uint32_t nrc_cache_get_infer_batch_size(nrc_cache_t* c);
uint32_t nrc_cache_get_train_batch_size(nrc_cache_t* c);

/* --- finer-grained steps of the same path (what InferAndTrain is made of; used by the multi-GPU driver) --- */
/* network->inference on an arbitrary device buffer (src/NeuralRadianceCache.cu:142); use_ema=1 is what Inference does */
int nrc_cache_infer(nrc_cache_t* c, const float* d_input, float* d_output, uint32_t n, int use_ema);
/* trainer->training_step minus the optimizer (src/NeuralRadianceCache.cu:153): forward (non-EMA weights) + loss + backward.
 * n_norm: batch size the loss normaliser uses (= n on one GPU, the global batch when the batch is sharded). */
int nrc_cache_backward(nrc_cache_t* c, const float* d_input, const float* d_target, uint32_t n, uint32_t n_norm);
/* optimizer step (EMA{Adam}) from the gradient vector */
int nrc_cache_optimizer_step(nrc_cache_t* c);
/* device pointer / length of the fp32 gradient vector (sum over the local batch, times loss_scale 128) and of the
 * 2-float {loss, unused} cell, which directly follows the gradient vector in memory (loss_ptr == grad_ptr +
 * param_count): the multi-GPU driver all-reduces param_count + 2 floats between backward and optimizer_step.  From the first
 * call on, nrc_cache_optimizer_step reads this vector for EVERY parameter (a HashGrid table's gradient otherwise comes from the
 * packed fp16 table the backward pass accumulated into; unmodified, the vector holds the same values) */
float* nrc_cache_grad_ptr(nrc_cache_t* c);
uint32_t nrc_cache_param_count(nrc_cache_t* c);
float* nrc_cache_loss_ptr(nrc_cache_t* c);
/* multi-GPU, native exchange: rank 0 obtains a 128-byte RCCL unique id (nrc_comm_unique_id), distributes it, and every
 * rank calls nrc_cache_comm_init(id, rank, world) (collective).  From then on every train batch all-reduces (sum) the
 * gradient vector + loss cell with ncclAllReduce on the training stream and normalises the loss by the global batch. */
int nrc_comm_unique_id(void* out128);
int nrc_cache_comm_init(nrc_cache_t* c, const void* unique_id128, int rank, int world);
/* What travels in that exchange (BASELINE.json configs[3]: "RCCL fp16 grad all-reduce"; SURVEY.md 8e recommends both):
 *   NRC_EXCHANGE_F32 (default)  the fp32 gradient vector + loss cell, one ncclAllReduce(ncclFloat) of param_count + 2 words (103 KB for 6 x 64)
 *   NRC_EXCHANGE_F16            the gradients as tiny-cuda-nn holds them -- fp16, pre-scaled by loss_scale 128 (the local sum is accumulated in
 *                               fp32 and rounded ONCE) -- summed by ncclAllReduce(ncclHalf) (52 KB), widened back into the fp32 vector the
 *                               optimizer reads; the loss cell stays fp32, grouped with it.  A HashGrid model's matrices travel the same way,
 *                               its table lists carry fp16 values in either mode.  Replicas stay bit-identical (every rank receives the same
 *                               sum).  A gradient hook (nrc_cache_set_grad_hook) is handed fp16-rounded values in the fp32 vector and its
 *                               result is rounded again: for two ranks exactly the fp16 sum.
 * Set on every rank alike, before the first training step; nrc_cache_get_exchange_dtype returns the mode in use. */
#define NRC_EXCHANGE_F32 0
#define NRC_EXCHANGE_F16 1
int nrc_cache_set_exchange_dtype(nrc_cache_t* c, int dtype);
int nrc_cache_get_exchange_dtype(nrc_cache_t* c);
/* Training guard: what a training step does whose loss or gradient is not finite (one NaN target, a self-training tail from a diverging
 * cache, an fp16 exchange whose sum passes 65 504).  A per-cache policy:
 *   NRC_NONFINITE_PROPAGATE (default)  the optimizer applies the step: weights, EMA weights and Adam moments become non-finite, the caller
 *                                      learns it from the loss it polls.  Every result is bit for bit what it was without the guard.
 *   NRC_NONFINITE_SKIP                 every training batch gets a verdict on the device, on the training stream, behind the gradient exchange
 *                                      (RCCL all-reduce, fp16 exchange, list exchange, gradient hook, a caller's own reduction of
 *                                      nrc_cache_grad_ptr) and in front of the optimizer's first write.  The step is BAD when
 *                                        1. the loss cell loss[0] -- behind the exchange: the global loss -- is not finite, or
 *                                        2. one of the first n_mlp (matrix) words of the gradient vector the optimizer is about to read is not
 *                                           finite (exponent bits all ones).
 *                                      The HashGrid table gradient is not scanned: its entries are fp16 / fixed-point sums of per-ray terms that
 *                                      can only leave the finite range together with the loss, and in the list exchange every rank's loss is
 *                                      summed into the cell: rule 1 covers it.
 * Both inputs of the verdict are bits every rank holds identically behind the exchange (what keeps the replicas identical in the first place), so
 * every rank reaches the same verdict with no further collective.  Set the policy on every rank alike.
 * A bad step
 *   - leaves master weights, EMA weights and Adam m / v (table entries included) exactly as they were;
 *   - still writes the fp16 images of the next inference set, from the unchanged weights (the host alternates the sets whatever the verdict);
 *   - still publishes its (non-finite) loss and sequence number: nrc_cache_get_loss / nrc_cache_get_loss_async keep their meaning;
 *   - still consumes its step number.  The host never learns a verdict in time and does not wait for one, and it computes the bias corrections of
 *     Adam and of the EMA from the step number.  The contract therefore is: A SKIPPED STEP IS A STEP WHOSE UPDATE IS THE IDENTITY; THE BIAS
 *     CORRECTIONS COUNT ENQUEUED STEPS.  (An approximation against an optimizer that would not count it: Adam's lr_t differs by 0.5 % at step
 *     100, less later.)  A run with a skipped step k equals, bit for bit, the run without that batch and nrc_cache_set_step(k) in its place;
 *   - increments a device-resident counter and records its step number (nrc_cache_get_step's value for that step).
 * A good step under SKIP produces the bits it produces under PROPAGATE.  Cost: the scan rides on the pass that writes the final gradient where there
 * is one (the gradient reduction without an exchange, the last pass of the fp16 exchange); behind an fp32 all-reduce, an fp32 hook or a caller's
 * own reduction it is one launch over n_mlp words.
 * The policy may be changed between steps; that does not reset the counter.  Checkpoints do not carry the counter.
 * nrc_cache_get_skipped_steps: *skipped = steps skipped since the cache was created, *last_skipped_step = step number of the latest (0: none);
 * waits for the last enqueued training step only, like nrc_cache_get_loss. */
#define NRC_NONFINITE_PROPAGATE 0
#define NRC_NONFINITE_SKIP 1
int nrc_cache_set_nonfinite_policy(nrc_cache_t* c, int policy);
int nrc_cache_get_nonfinite_policy(nrc_cache_t* c);
int nrc_cache_get_skipped_steps(nrc_cache_t* c, uint32_t* skipped, uint32_t* last_skipped_step);
/* rank / size as the library's own RCCL communicator reports them (ncclCommUserRank / ncclCommCount); world = 0: none */
int nrc_cache_comm_info(nrc_cache_t* c, int* rank, int* world);
/* Failure detection on the exchange ("RCCL error -> status code").  An enqueued collective reports nothing by itself:
 * every call into the library that uses the communicator first polls ncclCommGetAsyncError (non-blocking), and every wait of the library
 * for work that sits behind a collective -- the frame gather, the sharded metrics, nrc_cache_get_loss_blocking, the collective export --
 * has a deadline (default 30 000 ms once the frame has more than one rank; 0 = wait for ever).  On an asynchronous error, a collective
 * hook that returns non-zero, or a missed deadline the communicator is aborted (ncclCommAbort: its kernels are killed, nothing is left
 * hanging on the streams), the call returns NRC_ERR_COMM with the reason, and so does every later call that would need the exchange;
 * the ranks that still work see the same through their own deadline.  nrc_cache_comm_status: NRC_OK, or NRC_ERR_COMM (polls, never blocks). */
int nrc_cache_comm_status(nrc_cache_t* c);
int nrc_cache_set_comm_timeout_ms(nrc_cache_t* c, uint32_t ms);
/* measurement: *avg_us = average duration of the training step's ncclAllReduce (gradient vector + loss cell, zeroed first), issued
 * `reps` times back to back on the cache's stream; collective -- every rank calls it with the same reps.  0 without a communicator. */
int nrc_cache_comm_time_exchange(nrc_cache_t* c, uint32_t reps, float* avg_us);
/* HashGrid models (posID 0): the trainable table's gradient -- 57 MB dense, a few per cent of it touched by a batch -- is
 * exchanged as all-gathered (entry, fp16x2 value) lists that every rank adds in rank order (replicas stay bit-identical), the
 * matrix gradients and the loss cell by ncclAllReduce as before.  Chosen at nrc_cache_comm_init when world x list capacity
 * (trainBatchSize x 16 levels x 8 corners, at most the table) < 2 x table entries, i.e. when the padded all-gather moves less
 * than the ring all-reduce; environment NRC_DEBUG=dense_grid_exchange forces the dense exchange.  nrc_cache_comm_sparse: 1 when the list exchange is the one in use.  The two debug entry points expose its
 * halves on one device (tests): the list of the last nrc_cache_backward -- words {count, 0, (entry, value) x capacity},
 * padding entries 0xffffffff, list_words >= 2 + 2 * nrc_cache_grid_list_capacity() -- and the gradient vector's table part
 * := sum of n_lists such lists (2 + 2 * capacity words apart), added in list order. */
int nrc_cache_comm_sparse(nrc_cache_t* c);
size_t nrc_cache_grid_list_capacity(nrc_cache_t* c);
int nrc_cache_grid_grad_pack(nrc_cache_t* c, uint32_t* host_list, size_t list_words);
int nrc_cache_grid_grad_apply(nrc_cache_t* c, const uint32_t* host_lists, uint32_t n_lists);
/* multi-GPU: the loss normaliser of InferAndTrain's train batches becomes 3 * trainBatchSize * factor (factor = world size) */
int nrc_cache_set_loss_norm_factor(nrc_cache_t* c, uint32_t factor);
/* move the cache's work to another hipStream_t (Init binds the first one) */
int nrc_cache_set_stream(nrc_cache_t* c, void* stream);
/* hook called between backward and the optimizer of every train batch (NULL = none); `stream` is the hipStream_t the
 * training kernels are ordered on -- the exchange (all-reduce) must be issued on it */
typedef void (*nrc_grad_hook)(void* user, float* d_grad, uint32_t n_params, float* d_loss, void* stream);
int nrc_cache_set_grad_hook(nrc_cache_t* c, nrc_grad_hook hook, void* user);
/* Collectives of a multi-GPU frame that are NOT the gradient exchange -- the frame gather and the metric reduction below -- go through
 * the communicator nrc_cache_comm_init made; a cache without one can be given the caller's transport instead (the tests' gloo
 * rehearsal, a host that brings MPI): allreduce sums n doubles in place over all ranks, allgather fills d_recv = [world][bytes_per_rank]
 * with every rank's d_send; both work on device memory and return 0 on success.  The library has waited for `stream` (a hipStream_t)
 * when it calls a hook, so a transport that stages through host memory may read the buffers at once; what the hook writes must be
 * complete, or ordered on `stream`, when it returns. */
typedef int (*nrc_allreduce_f64_fn)(void* user, double* d_buf, uint32_t n, void* stream);
typedef int (*nrc_allgather_fn)(void* user, const void* d_send, void* d_recv, size_t bytes_per_rank, void* stream);
int nrc_cache_set_collective_hooks(nrc_cache_t* c, int rank, int world, nrc_allreduce_f64_fn allreduce, nrc_allgather_fn allgather, void* user);
/* checkpointing: which = 0 master weights, 1 EMA weights, 2 Adam m, 3 Adam v, 4 gradient (host fp32 arrays) */
int nrc_cache_get_params(nrc_cache_t* c, int which, float* host_out);
int nrc_cache_set_params(nrc_cache_t* c, int which, const float* host_in);
/* the same vectors in tiny-cuda-nn v1.6's OWN parameter layout -- what a dump of its Trainer's params_full_precision holds for the model
 * tcnn::create_from_config(5, 3, cfg) builds at src/NeuralRadianceCache.cu:39, so that weights saved from the reference can be loaded
 * (and the other way round): the matrices in the same order and row-major orientation, the output matrix with its rows padded to 16
 * (16 x nnWidth; rows 3..15 feed the padded outputs nobody reads: kept on the host as initialised / last set, never trained), then the
 * encoding's table.  count = nrc_cache_param_count + 13 * nnWidth (26 624 for the 6 x 64 model with the 80-wide encoding). */
uint32_t nrc_cache_param_count_tcnn(nrc_cache_t* c);
int nrc_cache_get_params_tcnn(nrc_cache_t* c, int which, float* host_out);
int nrc_cache_set_params_tcnn(nrc_cache_t* c, int which, const float* host_in);
/* checkpoint FILE (the reference has none; SURVEY.md section 5 "checkpoint / resume"): little-endian, 64-byte header {"NRCCKPT1", posID,
 * dirID, nnWidth, nnDepth, hashgrid log2 size, tcnn parameter count, optimizer step, 0...} + the four vectors which = 0..3 in the
 * tiny-cuda-nn layout above.  load checks the header against the cache's model (NRC_ERR_INVALID on a mismatch, a short or unreadable
 * file) and leaves the cache untouched on failure. */
int nrc_cache_save_checkpoint(nrc_cache_t* c, const char* path);
int nrc_cache_load_checkpoint(nrc_cache_t* c, const char* path);
int nrc_cache_get_step(nrc_cache_t* c, uint32_t* step);
int nrc_cache_set_step(nrc_cache_t* c, uint32_t step);

/* ---------------------------------------------------------------------------------------------------------
 * Scene inputs: the values the reference uploads as UBOs / textures.  HOST pointers; copied
 * to the device at renderer creation. */
typedef struct nrc_scene {
    const uint8_t* density;        /* R8 UNORM voxels, index i + nx*(j + ny*k)  (src/Texture3D.cpp:99-111, one channel) */
    uint32_t nx, ny, nz;
    float size[3];                 /* skySize; all zero => normalize(extent)*107.5 (src/NrcHpmRenderer.cu:910-912) */
    float density_factor;          /* VolumeData density (scene preset) */
    float g;                       /* 0.8 (src/HpmScene.cpp:45) */
    float dir_light_dir[3];        /* src/DirLight.cpp:5-14 */
    float dir_light_strength;
    float point_light_pos[3];
    float point_light_strength;
    float point_light_color[3];
    float env_strength;
    const float* env;              /* RGBA32F row-major env_h x env_w (src/HdrEnvMap.cpp), LINEAR clamp-to-edge */
    uint32_t env_w, env_h;
} nrc_scene;

/* CameraMatrices.invProjView + camera.pos (include/engine/graphics/Camera.hpp:11-16, nrc-descriptors.glsl:1-11) */
typedef struct nrc_camera {
    float inv_proj_view[16];       /* column-major (glm) */
    float pos[3];
} nrc_camera;

/* Pixel-tile shard of a frame (new: SURVEY.md section 8e).  This instance renders strips of x_block adjacent columns of a
 * global_w x global_h frame, every x_stride-th strip starting with strip x_offset: local column i (i = 0..width-1) is the global
 * column (x_offset + (i / x_block) * x_stride) * x_block + i % x_block; width passed to create is the LOCAL column count.
 * x_block must be a power of two; 0 means 1 (single interleaved columns).  {0,1,W,H,0} = whole frame.  Strips of 8 columns keep
 * the 8x8-pixel tile a wavefront renders contiguous on the screen (coherent walks, as on one GPU) at the same load balance.
 * ABI note: the struct has FIVE fields (20 bytes) since nrc_version() "0.2"; "0.1" had four (16 bytes, no x_block) -- a caller built
 * against the older header must be recompiled (the library would read x_block past the end of its struct). */
typedef struct nrc_tile {
    uint32_t x_offset, x_stride, global_w, global_h;
    uint32_t x_block;
} nrc_tile;

/* ---------------------------------------------------------------------------------------------------------
 * en::NrcHpmRenderer (include/engine/graphics/renderer/NrcHpmRenderer.hpp:13-41, src/NrcHpmRenderer.cu) */
typedef struct nrc_renderer nrc_renderer_t;

/* NrcHpmRenderer(width, height, blend, camera, appConfig, hpmScene, nrc) (src/NrcHpmRenderer.cu:212-297).
 * The renderer allocates the four NRC I/O buffers and calls nrc_cache_init (as the reference ctor does, :259-266).
 * tile may be NULL.  Creation also builds the host-side index of the pixels' RNG seeds that the hot-tile search uses (see
 * nrc_renderer_set_hot_tiles): one hash per pixel and 4 bytes per pixel + 3 MB of host memory -- 84 ms and 11 MB at 1920x1080,
 * about 0.5 s and 43 MB at 3840x2160 -- whether or not a frame ever uses it; nrc_mc_renderer_create does the same. */
int nrc_renderer_create(uint32_t width, uint32_t height, int blend, const nrc_camera* camera, const nrc_config* cfg,
                        const nrc_scene* scene, nrc_cache_t* cache, const nrc_tile* tile, void* stream,
                        nrc_renderer_t** out);
/* NrcHpmRenderer::Render(VkQueue, bool train) (src/NrcHpmRenderer.cu:299-353) */
int nrc_renderer_render(nrc_renderer_t* r, int train);
/* n_frames consecutive Render(queue, train) calls enqueued by ONE call (the host loop of src/main.cu:287 without a trip through the
 * binding per frame); frame_randoms: n_frames x 4 floats, frame f's UniformData.random (NULL: the renderer draws them, as Render does) */
int nrc_renderer_render_frames(nrc_renderer_t* r, uint32_t n_frames, const float* frame_randoms, int train);
/* NrcHpmRenderer::SetCamera / SetBlend (src/NrcHpmRenderer.cu:561-610) */
int nrc_renderer_set_camera(nrc_renderer_t* r, const nrc_camera* camera);
/* A camera path (a turntable, a fly-through; the reference has no equivalent): n_cameras views of frames_per_camera frames each,
 * enqueued by one call that does not wait for the GPU.  It computes, bit for bit, what this loop computes --
 *     for i in 0 .. n_cameras-1:  set_camera(cameras[i]);
 *                                 for k in 0 .. frames_per_camera-1:  [set_frame_random(frame_randoms + 4*(i*fpc + k))]  render(train)
 *                                 copy the framebuffer to d_frames + i*h*w*4
 * -- framebuffer, d_frames and, with train, the cache's loss, weights, optimizer state, step and training ring; but where set_camera
 * waits for every frame in flight, a view here starts behind the previous one on the device: the frames in flight keep their camera,
 * blending restarts at every view, the accumulation image is cleared behind the previous view's last compositing and copy, and the
 * empty-space tile mask of the view is built by kernels that run in parallel over the mask (the same words as set_camera's mask).
 *   cameras        host memory, n_cameras entries.
 *   frame_randoms  n_cameras * frames_per_camera * 4 host floats, or NULL: the renderer draws them, in the sequence that many
 *                  consecutive Render calls would.
 *   d_frames       device memory, [n_cameras][h][w][4] RGBA32F (local columns of a sharded renderer), or NULL: only the last view
 *                  stays, in the framebuffer.  View i is copied on the stream of its last compositing, behind it.  When the call returns
 *                  the stream given at creation has been made to wait, on the device, for the last copy: work enqueued on that stream
 *                  afterwards sees all of d_frames (the contract of nrc_renderer_framebuffer).
 * n_cameras == 0 is a no-op; otherwise cameras == NULL or frames_per_camera == 0 returns NRC_ERR_INVALID and leaves the renderer
 * unchanged.  No hipStreamSynchronize, no blocking copy -- with two exceptions that are not the path's: a renderer's very first tile
 * mask reads 36 bytes back (the selection of capped RNG states, kept from then on), and while the schedule tuner plays a trial Render
 * bounds the host's run-ahead.  The tuner discards a trial window that contains a view change (no schedule measured across views reaches
 * the schedule cache) and starts its trials again 128 frames after the path's last view change.  The first path of a renderer allocates 8 bytes per
 * empty-space box.  In a sharded run every rank makes the same call. */
int nrc_renderer_render_path(nrc_renderer_t* r, uint32_t n_cameras, const nrc_camera* cameras, uint32_t frames_per_camera,
                             const float* frame_randoms, int train, float* d_frames);
/* diagnostics: the empty-space tile mask in use after synchronising: n = nrc_renderer_tile_mask(r, NULL, 0) words
 * (ceil(tiles / 32) bit words, tile ty * ceil(w / 8) + tx at bit id % 32 of word id / 32, + the trailing "mask off for this camera"
 * word); 0 words when the frame uses no mask (empty skip off, no perspective camera, a medium too dense for it) */
size_t nrc_renderer_tile_mask(nrc_renderer_t* r, uint32_t* host_out, size_t capacity);
/* diagnostics: the far bounds built with that mask, one float per tile (index ty * ceil(w / 8) + tx): an upper bound of the distance from
 * the camera position behind which no camera ray of the tile meets density again (DESIGN.md section 4.4 "Far cut"; 0: no occupancy box
 * touches the tile).  Same calling pattern; 0 floats when the frame uses no mask. */
size_t nrc_renderer_tile_far(nrc_renderer_t* r, float* host_out, size_t capacity);
int nrc_renderer_set_blend(nrc_renderer_t* r, int blend);
/* The uniform-buffer half of the scene -- DirLight / PointLight / VolumeData / HdrEnvMap strength (src/DirLight.cpp:31-49,
 * src/HpmScene.cpp:56-76 `HpmScene::Update`, the ImGui light editors): takes effect with the next Render and does not reset
 * blending (only a camera change does, src/NrcHpmRenderer.cu:561-604).  The density volume and the environment map of `scene`
 * are ignored: the environment map is fixed at creation, a new density volume goes in with nrc_renderer_set_volume. */
int nrc_renderer_set_scene_params(nrc_renderer_t* r, const nrc_scene* scene);
/* Replace the density volume of a live renderer (animated media; the reference has no equivalent).  density: nx*ny*nz voxels, index
 * i + nx*(j + ny*k) (a [nz][ny][nx] array), the dims the renderer was created with (otherwise NRC_ERR_INVALID and the renderer is
 * unchanged).  format NRC_VOLUME_U8: R8 UNORM, taken as is; NRC_VOLUME_F32: float, quantised as the reference does, uint8(v * 255)
 * truncated, with v <= 0 and NaN -> 0 and v >= 1 -> 255.  The density, the occupancy bits and the empty-space boxes are rebuilt on the
 * device; world size, density factor, lights and the environment map stay as they are.
 *   on_device = 1: density is device memory, read on the stream given at creation -- the call does not wait for the GPU, and the caller
 *     may overwrite the buffer with work it enqueues on that stream afterwards.
 *   on_device = 0: density is host memory; the call copies it and returns when the copy is done (it waits for that stream).
 * Frames enqueued before the call render the old volume, frames enqueued after it the new one.  Progressive blending resets (as
 * set_camera); the cache's weights, optimizer state and training ring are kept: following the change is the online training's job.
 * In a sharded run every rank calls it, with the whole volume, before the same frame. */
#define NRC_VOLUME_U8 0
#define NRC_VOLUME_F32 1
int nrc_renderer_set_volume(nrc_renderer_t* r, const void* density, uint32_t nx, uint32_t ny, uint32_t nz, int format, int on_device);
/* The same replacement from a sparse source: n_bricks bricks of 8 x 8 x 8 voxels (the leaf size of a VDB tree and the cell size of the
 * renderer's empty-space boxes).  origins[3*i .. 3*i+2] is the voxel coordinate (x0, y0, z0) of brick i's first voxel; bricks holds
 * n_bricks * 512 elements, voxel (x0+dx, y0+dy, z0+dz) of brick i at element 512*i + 64*dz + 8*dy + dx (an [8][8][8] array, x fastest,
 * like the dense [nz][ny][nx]); format and its quantisation rule as above.  The volume keeps the dims of creation (they are not passed).
 *   Whole replacement: every voxel no brick covers becomes 0, whatever the volume held before.  Brick voxels past the volume's edge are
 *     ignored (the dims need not be multiples of 8); a brick of zeros is legal and leaves its cell empty; n_bricks = 0 (the pointers
 *     may be NULL) is the empty medium.  When several bricks name one cell, the one with the highest index wins, deterministically.
 *   An origin is valid when every component is a multiple of 8 and 0 <= x0 < nx, 0 <= y0 < ny, 0 <= z0 < nz.  A host list is checked:
 *     a violation returns NRC_ERR_INVALID, the message names the brick, and the renderer is unchanged.  A device list cannot be
 *     checked without a wait: a brick with an invalid origin is ignored on the device, and nothing is written out of bounds.
 *   on_device applies to both pointers, as above: device memory is read on the creation stream and the call does not wait for the GPU;
 *     host memory is copied (12*n + 512*n*element size bytes) and the call returns when the copy is done.  The vector loads of the
 *     rebuild need bricks aligned to 4 elements (device memory; any allocation is); an unaligned pointer is read element by element.
 * Everything else is as for nrc_renderer_set_volume: the order against frames enqueued before and after, the blending reset, what is
 * kept (cache, optimizer state, training ring, schedule key), and in a sharded run every rank calls it with the whole list.  Dense and
 * brick calls may be mixed freely.  The device buffers are the rebuild of the densified list, bit for bit. */
int nrc_renderer_set_volume_bricks(nrc_renderer_t* r, const int32_t* origins, const void* bricks, uint32_t n_bricks, int format, int on_device);
/* Volume keyframes (retiming a cached simulation, slow motion, an animated fly-through; the reference has no equivalent): a sequence
 * of key volumes resident on the device, and the renderer's medium set to the linear in-between of two of them.
 *   Keys.  A renderer holds n_keys key volumes; key i sits at time i.  volumes is one contiguous [n_keys][nz][ny][nx] array of `format`
 *     with the dims the renderer was created with; the library keeps its own copy on the device as R8 (n_keys * nx*ny*nz bytes).  A
 *     NRC_VOLUME_F32 source is quantised once, at upload, by the rule of nrc_renderer_set_volume: exactly the bytes that call would have
 *     written.  on_device = 0: host memory, the call copies and returns when the copy is done; on_device = 1: device memory, read on the
 *     stream given at creation, and the call does not wait for that read.  n_keys = 0 drops the sequence (the other arguments are then
 *     ignored).  Replacing or dropping a sequence may wait for every stream of the renderer (the frames in flight may read the old
 *     keys): this is NOT a per-frame call.  The renderer's current medium is not touched.  A call that fails -- other dims, volumes ==
 *     NULL, an unknown format, an allocation failure -- leaves the renderer and the previous keys as they were.
 *   Time -> key pair and weight.  t must be finite and inside [0, n_keys - 1]; otherwise NRC_ERR_INVALID, and nothing is enqueued
 *     (no keys: every t fails).  i = min((uint32)t, n_keys - 1); w = t - (float)i in fp32; W = (uint32)(w * 256.0f + 0.5f), so
 *     0 <= W <= 256, and W = 0 at the last key.
 *   The in-between voxel is integer arithmetic, bit-exact on every machine: with a, b the R8 voxels of keys i and i + 1,
 *         q = (a * (256 - W) + b * W + 128) >> 8.
 *     W = 0 gives a and W = 256 gives b; q lies between a and b, so the majorant (density_factor, texture <= 1) stays valid.  A voxel
 *     of 1 fading to 0 is 1 up to W = 128 and 0 from W = 129: the occupancy bits and the empty-space boxes follow q, not the keys.
 *   nrc_renderer_set_volume_time(t) is, by definition, nrc_renderer_set_volume(the in-between volume of t, NRC_VOLUME_U8, on_device = 1):
 *     the same slot swap, the same three device buffers byte for byte (nrc_renderer_volume_buffer), the same blending restart, the
 *     cache's weights, optimizer state and ring kept, and no host wait.  The in-between is blended straight into the slot.
 *   nrc_renderer_render_path_timed is nrc_renderer_render_path with a time per view: it computes, bit for bit, what
 *         set_volume_time(times[i]); set_camera(cameras[i]); frames_per_camera x render(train); copy to d_frames + i*h*w*4
 *     per view computes (framebuffer, images and, with train, loss, weights, optimizer state, step and ring), enqueued by one call that
 *     does not wait for the GPU.  times: n_cameras host floats, every one checked before the first view is enqueued (one bad time:
 *     NRC_ERR_INVALID, nothing rendered); times == NULL is nrc_renderer_render_path.  A view whose (i, W) is what the sequence last put
 *     into the renderer (by set_volume_time or a timed path, with no set_volume / set_volume_bricks / set_volume_keys call since) skips
 *     the rebuild -- the result cannot differ; (i, 256) and (i + 1, 0) count as the same.  Everything else as for nrc_renderer_render_path.
 *   In a sharded run every rank makes the same calls with the same keys and times. */
int nrc_renderer_set_volume_keys(nrc_renderer_t* r, const void* volumes, uint32_t n_keys, uint32_t nx, uint32_t ny, uint32_t nz, int format,
                                 int on_device);
uint32_t nrc_renderer_volume_key_count(nrc_renderer_t* r);
int nrc_renderer_set_volume_time(nrc_renderer_t* r, float t);
int nrc_renderer_render_path_timed(nrc_renderer_t* r, uint32_t n_cameras, const nrc_camera* cameras, const float* times,
                                   uint32_t frames_per_camera, const float* frame_randoms, int train, float* d_frames);
/* Sparse volume keyframes: the same key sequence held as lists of 8^3 bricks instead of dense volumes (a cached simulation whose frames
 * are mostly empty).  A renderer holds ONE key sequence, dense or bricks: setting either kind replaces whatever was there, and
 * nrc_renderer_volume_key_count, nrc_renderer_set_volume_time and nrc_renderer_render_path_timed work on either kind with the contracts
 * stated above.
 *   Keys.  key_counts: n_keys words, ALWAYS host memory -- key k is a list of key_counts[k] bricks.  origins and bricks are the keys' lists
 *     concatenated in key order, in the layouts of nrc_renderer_set_volume_bricks (origins int32[3 * total], bricks total * 512 elements of
 *     `format`, total = the sum of key_counts); on_device applies to these two pointers, as there.  The volume keeps the dims of creation.
 *     Per key the rules of nrc_renderer_set_volume_bricks hold: the highest index wins a cell named twice, a brick of zeros is legal, brick
 *     voxels past the volume's edge are ignored, a key with count 0 is the empty medium (total = 0: both pointers may be NULL).  A host list
 *     is checked: an invalid origin returns NRC_ERR_INVALID and the message names the key and the brick inside that key's list.  A device
 *     list's invalid origins are ignored on the device.  n_keys = 0 drops the sequence (the other arguments are then ignored).
 *   What is kept.  One R8 array of all bricks (a NRC_VOLUME_F32 source is quantised once, at upload, by the rule of
 *     nrc_renderer_set_volume) and, per key, one 32-bit word per 8^3 cell of the volume that names the cell's brick.  The origins are not
 *     kept.  nrc_renderer_volume_key_bytes returns the device bytes the current sequence holds:
 *         dense keys:  n_keys * nx*ny*nz
 *         brick keys:  512 * (sum of key_counts) + 4 * n_keys * cells,  cells = ceil(nx/8) * ceil(ny/8) * ceil(nz/8)
 *         no keys:     0
 *   Definition.  With brick keys, nrc_renderer_set_volume_time(t) leaves the three device buffers (nrc_renderer_volume_buffer) byte for
 *     byte what nrc_renderer_set_volume_keys(the densified keys) followed by nrc_renderer_set_volume_time(t) leaves, where the densified
 *     key is what nrc_renderer_set_volume_bricks makes of that key's list; the frames and the training that follow are therefore
 *     bit-identical too.  A cell with a brick in only one key blends against 0: for 0 < W < 256 that is NOT a copy of the brick (a voxel
 *     of 1 is 1 up to W = 128 and 0 from W = 129), and the occupancy follows q, not the keys.
 *   As nrc_renderer_set_volume_keys, the call may wait for every stream of the renderer: this is NOT a per-frame call.  The renderer's
 *     current medium is not touched.  A call that fails -- a NULL pointer, an unknown format, an invalid host origin, sizes that do not fit,
 *     an allocation failure -- leaves the renderer and the previous sequence, of either kind, as they were: the new sequence is complete
 *     before the old one goes.  In a sharded run every rank makes the same calls with the same lists. */
int nrc_renderer_set_volume_key_bricks(nrc_renderer_t* r, const uint32_t* key_counts, const int32_t* origins, const void* bricks, uint32_t n_keys,
                                       int format, int on_device);
size_t nrc_renderer_volume_key_bytes(nrc_renderer_t* r);
/* diagnostics: the current volume's device buffers after synchronising the renderer -- which 0: density [nz][ny][nx] u8, 1: occupancy
 * bits (uint32 words), 2: empty-space boxes float[6 * n] {lo.xyz, hi.xyz}; *bytes = their size (NULL, bytes 0: no boxes) */
const void* nrc_renderer_volume_buffer(nrc_renderer_t* r, int which, size_t* bytes);
/* UniformData.showNrc (include/engine/graphics/renderer/NrcHpmRenderer.hpp:70-75) */
int nrc_renderer_set_show_nrc(nrc_renderer_t* r, int show);
/* UniformData.random: by default drawn per frame from std::mt19937(seed) (the reference uses glm::linearRand,
 * src/NrcHpmRenderer.cu:308); this pins the next frame's value (parity tests) */
int nrc_renderer_set_frame_random(nrc_renderer_t* r, const float random4[4]);
/* GetImage()/GetImageView() -> device pointer, RGBA32F, row-major height x width (local columns).  The renderer composites
 * on an internal stream; this call makes the stream passed to nrc_renderer_create wait (on the device) for the latest frame's
 * compositing, so work enqueued on that stream afterwards sees the finished image.  Call it again after every Render. */
const float* nrc_renderer_framebuffer(nrc_renderer_t* r);
/* same image, but orders `consumer_stream` (a display or read-back stream of the caller) behind the latest compositing
 * instead of the render stream: reading every frame then does not hold back the next frame's ray generation.  Pair it with
 * nrc_renderer_release_frame once the reads are enqueued. */
const float* nrc_renderer_framebuffer_on(nrc_renderer_t* r, void* consumer_stream);
/* The framebuffer is ONE image that every frame's compositing blends in place (as the reference's m_OutputImage).  A consumer
 * that reads it on a stream of its own (framebuffer_on) must say when it is done: release_frame records the end of the reads
 * enqueued so far on consumer_stream, and the next frame's compositing waits for it on the device (nothing else of the next
 * frame does).  Without the call, a read that is still running when the next frame composites sees a torn image.
 * Not needed for nrc_renderer_framebuffer(): reads enqueued on the render stream are ordered before the next frame by
 * stream order. */
int nrc_renderer_release_frame(nrc_renderer_t* r, void* consumer_stream);
/* NrcHpmRenderer::IsBlending (include/engine/graphics/renderer/NrcHpmRenderer.hpp:37) */
int nrc_renderer_is_blending(nrc_renderer_t* r);
/* ExportOutputImageToFile (src/NrcHpmRenderer.cu:437-493): scan-line EXR, FLOAT RGBA */
int nrc_renderer_export_exr(nrc_renderer_t* r, const char* path);
/* Multi-GPU (new: SURVEY.md section 8e, "gather tiles to rank 0 or reduce only the metrics").  A frame sharded by nrc_tile is put
 * together again: every rank of the frame calls, every rank receives the whole [global_h][global_w] RGBA32F image in d_global_rgba
 * (device).  One all-gather of the ranks' column strips through the cache's communicator (nrc_cache_comm_init, or the hooks of
 * nrc_cache_set_collective_hooks) and a de-interleave kernel; bit-identical to the frame one GPU renders.  An unsharded renderer
 * copies its framebuffer.  export_exr_gathered is ExportOutputImageToFile (src/NrcHpmRenderer.cu:437-493) of such a run: collective,
 * rank `root` writes the file. */
int nrc_renderer_gather_frame(nrc_renderer_t* r, float* d_global_rgba, void* stream);
int nrc_renderer_export_exr_gathered(nrc_renderer_t* r, const char* path, int root);
/* EvaluateTimestampQueries + GetFrameTimeMS (src/NrcHpmRenderer.cu:495-530,556-559): synchronises; stage_ms may be
 * NULL or float[8] = {clear(0), gen_rays, prep_infer(0: fused into gen_rays), train, prep_train, inference, composite,
 * total}; with self-training, "train" includes the tail inference and the target combine in front of the backward pass.  The renderer pipelines frames over four streams (train-ray generation, training, inference + compositing of
 * frame N run beside gen_rays of frame N+1; DESIGN.md section 4 "Frame graph"), so the stages overlap, include the time they
 * wait for each other, and do not add up; total = latency of the frame, which exceeds the frame interval. */
float nrc_renderer_frame_time_ms(nrc_renderer_t* r, float* stage_ms);
/* the same stage times averaged over every frame rendered since the last reset (HIP events on the renderer's streams);
 * *frames = number of frames covered.  avg_ms == NULL with reset != 0 only forgets the frames so far, without reading an event */
int nrc_renderer_stage_stats(nrc_renderer_t* r, float avg_ms[8], uint32_t* frames, int reset);
/* Wave issue priority of the library's kernels (process-wide, current device): 1 (default) raises every kernel to s_setprio 3 -- no kernel of
 * the host can then outrank a path-integrator wave (the second guard behind the compiler flag) --, 0 leaves them all at
 * the hardware default.  Either way the whole library runs at ONE priority and the frame rate is the same; 0 is for a process whose
 * foreign kernels run beside the renderer (RCCL's all-reduce, the runtime's fills and copies): at priority 0 under waves at 3 a 28 MB
 * hipMemsetAsync took 184 us inside a frame, 65 us among equals.  nrc_cache_comm_init selects 0 for world > 1. */
int nrc_set_wave_priority_raise(int on);
/* the same events as a timeline (the reference's per-frame timestamp queries, src/NrcHpmRenderer.cu:495-515, kept for every frame since
 * the last reset): times_ms[f * 6 + k] = milliseconds from the first frame's start to event k of frame f -- 0 gen_rays starts, 1 gen_rays
 * done, 2 train rays done, 3 inference done, 4 compositing done, 5 training done -- for the first min(*frames, max_frames) frames;
 * synchronises, resets nothing.  Shows which stream a pipelined frame waits for (tools/frame_timeline.py). */
int nrc_renderer_frame_timeline(nrc_renderer_t* r, float* times_ms, uint32_t max_frames, uint32_t* frames);
/* NrcHpmRenderer::Destroy */
int nrc_renderer_destroy(nrc_renderer_t* r);
/* intermediate device buffers of the most recent frame, after synchronising all of the renderer's streams (tests /
 * multi-GPU; the sets rotate, so ask again after every Render): 0 primary colour+throughput [h][w][4], 1 primary info [h][w],
 * 2 nrc ray origin [h][w][4], 3 nrc ray dir [h][w][4] (train-grid pixels only unless set_full_vertex_images), 4 infer input [w*h][5], 5 infer output [w*h][3],
 * 6 train input [T][5], 7 train target [T][3], 8 train ring {head, tail, RayInfo[ring]}; self-training (nrc_config.self_train) of the
 * latest TRAINING frame, one entry per (ray i, sample s) at i * spp + s: 9 tail queries [T*spp][5] (zeros where there is no tail),
 * 10 {light.rgb, factor} [T*spp][4] (factor 0: no tail), 11 tail inference outputs [T*spp][3] (defined where there is a tail) --
 * NRC_ERR_INVALID for a renderer without self-training; 12 the frame's list of scattered pixels as gen_rays wrote it, uint32 {count,
 * indices[] in no particular order}, an index being ((y / 8) * ceil(w / 8) + x / 8) * 64 + (y % 8) * 8 + x % 8; the frame's compositing
 * pass has cleared the count for the set's next frame, the entries (as many as buffer 1 holds ones) stay -- NRC_ERR_INVALID for a
 * renderer that keeps no such list.  Buffers 4 and 5 are handed out in the
 * reference's order, query x*H+y (nrc/prep_infer_rays.comp:31), as a COPY made by this call: inside the renderer they are
 * tile-major (the 64 queries of an 8x8 pixel tile contiguous), and the cache's own API (nrc_cache_init / infer) speaks x*H+y
 * whatever its caller's order is.  Entries of pixels that did not scatter (info != 1) are zeros in both copies: the reference's zero-filled
 * query slots (src/NrcHpmRenderer.cu:1996), and a radiance nrc/render.comp:19-27 never reads -- the renderer's gen_rays and inference walk
 * the frame's list of scattered pixels and write nothing for the others. */
void* nrc_renderer_buffer(nrc_renderer_t* r, int which, size_t* bytes);
/* Empty-space early-out (on by default): camera rays that provably cannot come within a voxel of non-empty density skip their
 * delta-tracking walk -- the walk could only reject every tentative collision, leave the volume unscattered and produce env(rd),
 * and the RNG state behind it is never read, so the frame is bit-identical with and without (tests compare both against the
 * oracle, which always walks).  The 8x8-pixel tile mask behind it is rebuilt on the render stream whenever the camera changes.
 * on = 0 traces every ray (what count_fetches needs to report the ALGORITHM's look-ups rather than the executed ones). */
int nrc_renderer_set_empty_skip(nrc_renderer_t* r, int on);
/* Costliest-first launch order of gen_rays' 8x8-pixel tiles (on by default): every 16th frame records what each tile's wave cost,
 * a counting sort turns that into the order the following frames start their tiles in (the long walks through the cloud first,
 * the cheap rim in the tail of the launch).  The order is a permutation of the tiles and nothing else: frames are bit-identical
 * with and without.  tile_order copies the permutation in use (n = nrc_renderer_tile_order(r, NULL, 0) entries) to the host. */
/* The SCHEDULE of a renderer's frame graph: where and in which order work is placed -- no value changes a pixel or a weight (the tests render
 * under every combination and compare bit for bit).  The library chooses these itself: it starts from neutral values and, once the pipeline
 * has run for 128 frames, tries the alternatives on the caller's own frames against its frame timeline (one knob at a time, 24 frames per value,
 * the current value timed before and after the alternatives; ~250 frames in all) and keeps what is more than 1.5 % faster.  A caller that
 * knows better pins a knob with a value >= 0; -1 hands it (back) to the library.
 *   camera_priority_low  1: the camera kernels run at the default wave priority under the library's other kernels (pays where the
 *                        inference -> training chain bounds the frame: wide dense models), 0: at the common priority
 *   cost_order_lag       frames between a tile-cost sample and the first launch ordered by it (1..64; 2 or 3 are what the tuner tries)
 *   xcd_window           XCD-aware finish of the costliest-first launch order: tiles of a window of 32 x M ranks are dealt to the eight XCDs by
 *                        screen row (0 = off; the tuner tries 0, 2, 16); ignored on a device that does not have eight XCDs
 *   composite_defer      1: the compositing of the frames inside one nrc_renderer_render_frames call runs on the train-ray stream (not tuned) */
typedef struct nrc_schedule {
    int32_t camera_priority_low, cost_order_lag, xcd_window, composite_defer;
} nrc_schedule;
int nrc_renderer_set_schedule(nrc_renderer_t* r, const nrc_schedule* schedule);
/* the values in use now; *tuning_done (may be NULL) = 1 once nothing is left to choose */
int nrc_renderer_get_schedule(nrc_renderer_t* r, nrc_schedule* current, int* tuning_done);
/* Schedules survive the process.  What the tuner settles on is remembered in a process-wide table under a key that names everything the
 * choice depends on -- "<arch>:<CUs>cu:<XCDs>xcd|<model>|vol2^<log2 voxels>|<w>x<h>.of<global w>x<global h>|train<batches>x<rays>.len<train ray length>"
 * (nrc_renderer_schedule_key; a self-training renderer appends ".st": its frame graph has more work on the training stream) -- and a renderer created while its key is in the table starts on that schedule and skips the trials, so a run
 * shorter than the tuner's ~400 frames is a tuned run all the same.  nrc_schedule_cache_save writes the table (text: one "<key> <pri> <lag>
 * <window>" line per entry), nrc_schedule_cache_load merges a file into it (damaged lines are skipped; entries of other devices or models
 * simply never match); *n_entries (may be NULL) = entries read / written.  nrc_renderer_schedule_source says where the schedule in use came
 * from: "default" | "cache" | "tuner" (this renderer's own trials have ended) | "pinned" | "pinned in part".  The Python mirror loads
 * nrc-hpm-renderer_amd/schedules.txt (the tuner's results on this pool's MI355X for the BASELINE presets, tools/tune_schedules.py) with
 * the library (NRC_SCHEDULE_CACHE=<file> adds the host's own, NRC_SCHEDULE_CACHE="" loads none); a C++ host calls en::LoadScheduleCache(path). */
const char* nrc_renderer_schedule_source(nrc_renderer_t* r);
const char* nrc_renderer_schedule_key(nrc_renderer_t* r);
int nrc_schedule_cache_load(const char* path, int* n_entries);
int nrc_schedule_cache_save(const char* path, int* n_entries);
int nrc_schedule_cache_clear(void);      /* forget every entry (renderers created afterwards start on the defaults and tune) */
int nrc_renderer_set_cost_order(nrc_renderer_t* r, int on);
size_t nrc_renderer_tile_order(nrc_renderer_t* r, uint32_t* host_out, size_t capacity);
/* Hot tiles (on by default): a pixel whose RNG state can run into DeltaTrack's cap of 128 collisions inside a tile the empty-space
 * mask rejects (see set_empty_skip) is ONE lane that walks for ~0.12 ms; started where the launch order has its (empty) tile --
 * at the very end -- it ends the launch that much later (one frame in four on the bench view: mean 0.213 -> 0.232 ms).  The host
 * therefore finds those pixels when it enqueues a frame, for the random numbers the frame uses, by inverting the RNG's hash (about a
 * microsecond; the index of the pixels' seeds it uses is built when the renderer is created) and the launch starts up to 8
 * of their tiles first: no launch of its own, nothing read back.  Scheduling only: every tile is traced exactly once either way.
 * hot_tiles copies the last frame's list -- 8 entries (ty << 16 | tx), one per such pixel in pixel order, and their count -- from
 * host memory and returns 1 when the frame's random numbers were known when the frame before it was enqueued (the ones
 * render_frames was given, or drawn one frame early: same sequence), 0 when not (first frame, pinned random numbers), -1 when the
 * frame used none, -2 on error. */
int nrc_renderer_set_hot_tiles(nrc_renderer_t* r, int on);
int nrc_renderer_hot_tiles(nrc_renderer_t* r, uint32_t* host_out9);
/* The NRC vertex images (buffers 2 and 3: nrcRayOrigin / nrcRayDir of gen_rays.comp:97-100) are read back only at the pixels of
 * the train grid (prep_train_rays.comp:113-118), so by default gen_rays stores them only there; on != 0 makes it store every
 * pixel that entered the volume, as the reference's images hold (tests, debugging).  vertex_image_bytes: what one frame stores. */
int nrc_renderer_set_full_vertex_images(nrc_renderer_t* r, int on);
size_t nrc_renderer_vertex_image_bytes(nrc_renderer_t* r);
/* per-stage timing events (the reference's eight timestamp queries, src/NrcHpmRenderer.cu:495-530) of train-ray generation,
 * training, inference and compositing: on by default; off = four timed event records fewer per frame, frame_time_ms / stage_stats
 * then report gen_rays only */
int nrc_renderer_set_stage_events(nrc_renderer_t* r, int on);
/* density look-ups executed by gen_rays (measurement: algorithmic bytes of the integrator).
 * Returns the count accumulated so far in *out (may be NULL), then enables/disables + zeroes the device counter. */
int nrc_renderer_count_fetches(nrc_renderer_t* r, int enable, unsigned long long* out);
/* Of the look-ups counted above, those that ratio tracking kept from memory because their walk's transmittance was already exactly 0
 * and that the occupancy bits would have sent there: accumulated since count_fetches last zeroed the counters,
 * read before the next count_fetches call. */
int nrc_renderer_masked_fetches(nrc_renderer_t* r, unsigned long long* out);
/* The far cut's proof on the device, counted beside the look-ups (the counting launches walk every camera ray whole):
 * out[0] the camera walk's collisions at or behind the lane's cut in waves the cut applies to, out[1] those of them that met density (a
 * non-zero byte or an acceptance) -- 0 on every frame when the cut is sound.  Accumulated and read like masked_fetches. */
int nrc_renderer_cut_fetches(nrc_renderer_t* r, unsigned long long out[2]);
/* train grid chosen by CalcTrainSubset (src/NrcHpmRenderer.cu:612-642): {TW, TH, xDist, yDist, ringSize} */
int nrc_renderer_train_grid(nrc_renderer_t* r, uint32_t out5[5]);

/* ---------------------------------------------------------------------------------------------------------
 * en::McHpmRenderer (include/engine/graphics/renderer/McHpmRenderer.hpp:10-31, src/McHpmRenderer.cpp) */
typedef struct nrc_mc_renderer nrc_mc_renderer_t;

/* McHpmRenderer(width, height, pathLength, blend, camera, scene) (src/McHpmRenderer.cpp:81-119) */
int nrc_mc_renderer_create(uint32_t width, uint32_t height, uint32_t path_length, int blend, const nrc_camera* camera,
                           const nrc_scene* scene, const nrc_tile* tile, void* stream, nrc_mc_renderer_t** out);
/* McHpmRenderer::Render(VkQueue) (src/McHpmRenderer.cpp:121-151) */
int nrc_mc_renderer_render(nrc_mc_renderer_t* r);
int nrc_mc_renderer_set_camera(nrc_mc_renderer_t* r, const nrc_camera* camera);
int nrc_mc_renderer_set_blend(nrc_mc_renderer_t* r, int blend);
int nrc_mc_renderer_set_empty_skip(nrc_mc_renderer_t* r, int on);   /* see nrc_renderer_set_empty_skip */
int nrc_mc_renderer_set_cost_order(nrc_mc_renderer_t* r, int on);   /* see nrc_renderer_set_cost_order */
int nrc_mc_renderer_is_blending(nrc_mc_renderer_t* r);          /* include/engine/graphics/renderer/McHpmRenderer.hpp */
int nrc_mc_renderer_set_scene_params(nrc_mc_renderer_t* r, const nrc_scene* scene);   /* see nrc_renderer_set_scene_params */
/* see nrc_renderer_render_path (no train flag; one stream: views, frames and copies follow each other in stream order) and
 * nrc_renderer_tile_mask */
int nrc_mc_renderer_render_path(nrc_mc_renderer_t* r, uint32_t n_cameras, const nrc_camera* cameras, uint32_t frames_per_camera,
                                const float* frame_randoms, float* d_frames);
size_t nrc_mc_renderer_tile_mask(nrc_mc_renderer_t* r, uint32_t* host_out, size_t capacity);
size_t nrc_mc_renderer_tile_far(nrc_mc_renderer_t* r, float* host_out, size_t capacity);   /* see nrc_renderer_tile_far */
/* see nrc_renderer_set_volume / nrc_renderer_volume_buffer (one stream: the volume is rewritten in stream order behind the frames) */
int nrc_mc_renderer_set_volume(nrc_mc_renderer_t* r, const void* density, uint32_t nx, uint32_t ny, uint32_t nz, int format, int on_device);
/* see nrc_renderer_set_volume_bricks */
int nrc_mc_renderer_set_volume_bricks(nrc_mc_renderer_t* r, const int32_t* origins, const void* bricks, uint32_t n_bricks, int format, int on_device);
/* see nrc_renderer_set_volume_keys (no train flag in the timed path; one stream: rebuilds, views and copies in stream order) */
int nrc_mc_renderer_set_volume_keys(nrc_mc_renderer_t* r, const void* volumes, uint32_t n_keys, uint32_t nx, uint32_t ny, uint32_t nz, int format,
                                    int on_device);
uint32_t nrc_mc_renderer_volume_key_count(nrc_mc_renderer_t* r);
/* see nrc_renderer_set_volume_key_bricks */
int nrc_mc_renderer_set_volume_key_bricks(nrc_mc_renderer_t* r, const uint32_t* key_counts, const int32_t* origins, const void* bricks, uint32_t n_keys,
                                          int format, int on_device);
size_t nrc_mc_renderer_volume_key_bytes(nrc_mc_renderer_t* r);
int nrc_mc_renderer_set_volume_time(nrc_mc_renderer_t* r, float t);
int nrc_mc_renderer_render_path_timed(nrc_mc_renderer_t* r, uint32_t n_cameras, const nrc_camera* cameras, const float* times,
                                      uint32_t frames_per_camera, const float* frame_randoms, float* d_frames);
const void* nrc_mc_renderer_volume_buffer(nrc_mc_renderer_t* r, int which, size_t* bytes);
int nrc_mc_renderer_set_frame_random(nrc_mc_renderer_t* r, const float random4[4]);
const float* nrc_mc_renderer_framebuffer(nrc_mc_renderer_t* r);   /* RGBA32F, alpha = blended didScatter */
int nrc_mc_renderer_export_exr(nrc_mc_renderer_t* r, const char* path);
float nrc_mc_renderer_frame_time_ms(nrc_mc_renderer_t* r);
int nrc_mc_renderer_count_fetches(nrc_mc_renderer_t* r, int enable, unsigned long long* out);
int nrc_mc_renderer_destroy(nrc_mc_renderer_t* r);

/* ---------------------------------------------------------------------------------------------------------
 * Reference::Result metrics (include/engine/graphics/Reference.hpp:17-29, data/shader/ref/cmp1,norm,cmp2.comp):
 * device RGBA32F images of w*h pixels; result5 (host) = {mse, refMean, ownMean, ownVar, validPixelCount} */
int nrc_compare_images(const float* d_ref_rgba, const float* d_own_rgba, uint32_t w, uint32_t h, void* stream,
                       float result5[5]);

/* the same Result for a frame sharded over ranks (Reference::CompareNrc / CompareMc of a multi-GPU run, src/Reference.cpp:72-107):
 * every rank passes ITS pixels of the reference and of its image (n_local_pixels, any partition of the frame), the five sums are
 * formed locally in fp64 and summed over the ranks with two small all-reduces (4 + 1 doubles) through `comm`'s communicator; every
 * rank receives the whole frame's Result.  Equal to nrc_compare_images of the gathered frame up to the rounding of the fp64 sums. */
int nrc_compare_images_sharded(nrc_cache_t* comm, const float* d_ref_local_rgba, const float* d_own_local_rgba, uint32_t n_local_pixels,
                               void* stream, float result5[5]);

/* device-resident RGBA32F image [h][w] for nrc_compare_images: a copy of host_rgba (NULL: zeros) -- the reference image that
 * Reference::GenRefImages loads from reference/<scene>/0.exr into a VkImage (src/Reference.cpp:608-660) */
int nrc_image_create(uint32_t w, uint32_t h, const float* host_rgba, float** d_out);
int nrc_image_destroy(float* d_image);

/* ---------------------------------------------------------------------------------------------------------
 * View AOV: opacity and depth per pixel, exact for the medium (both renderers; every call has an nrc_mc_renderer_ twin).
 * A view AOV is an [h][w][4] fp32 image of {alpha, tau, z_front, z_half} per pixel; a sharded renderer holds its local columns, as its
 * framebuffer does.  It depends on the camera and the medium alone -- no random numbers, no frames -- and neither renderer's framebuffer
 * alpha changes (the NRC renderer's stays 1, the Monte-Carlo renderer's the blended scatter fraction, of which alpha is the expectation).
 *   Ray.     The pixel's camera ray is the one the frames trace: inv_proj_view applied to the frames' own fp32 u = global x / global_w,
 *            v = y / global_h (no half-pixel offset, no y flip), from camera.pos, normalised.  Distances t are along that ray from
 *            camera.pos.  The frames form the direction as (w.xyz / w.w) - pos in plain fp32, which at |pos| = 70 is 2e-5 rad from the
 *            ray of the fp32 matrix -- 1.5e-3 where it meets the medium, more than a depth should be off by.  The AOV evaluates the same
 *            expression with the large terms cancelled before anything is rounded (csrc/nrc_view_aov.hpp, view_aov_camera_ray): within
 *            5e-7 rad of that ray evaluated in fp64, and so within 3e-5 rad of the direction a frame's pixel traces.
 *   Density. sigma(p) = density_factor * u8 / 255 of the voxel that holds p (the frames' NEAREST look-up) inside the box, 0 outside:
 *            piecewise constant.  With t0 = max(0, box entry) and t1 = box exit,  tau = integral of sigma dt over [t0, t1].
 *   alpha    = 1 - exp(-tau).
 *   z_front  = the smallest t with sigma > 0.
 *   z_half   = the t at which the optical depth reaches ln 2, linear inside the voxel where it does; defined only when tau >= ln 2.
 *   An undefined depth is +inf.  A ray that misses the box or meets no non-empty voxel gives {0, 0, +inf, +inf}; so does every pixel
 *   of an 8x8 tile that the empty-space tile mask rejects (no ray of such a tile comes within a voxel of a non-empty one).
 *   No NaN for any finite camera; 0 <= alpha <= 1; 0 <= z_front <= z_half where both are finite.
 * The fp32 arithmetic is defined once, in csrc/nrc_view_aov.hpp, which the kernel and the host (nrc_test_view_aov_host) both run:
 *   voxel plane i of axis a lies at t_a(i) = fma(i, k_a, c_a), k_a = (size_a / n_a) / rd_a, c_a = (-size_a / 2 - ro_a) / rd_a -- from the
 *   plane's index, never a running sum; an axis with rd_a == 0 is never crossed, and the ray misses if |ro_a| >= size_a / 2; tau is
 *   accumulated front to back as fma(sigma_i, t_next - t_cur, tau); alpha = nrc_expm1_negf(tau) (csrc/nrc_math.h).  The result does not
 *   depend on how a traversal skips empty space (a skipped segment adds an exact 0), with or without the tile mask
 *   (nrc_renderer_set_empty_skip), and is bit-identical between the kernel and the host.
 * nrc_renderer_view_aov: the AOV of the current camera and medium (device memory, owned by the renderer, valid until the renderer is
 *   destroyed).  It is computed at most once per change of camera (set_camera, a path's views), volume (set_volume, set_volume_bricks,
 *   set_volume_time) or scene parameters, by one launch on the render stream behind the volume rebuilds and frames enqueued so far; no
 *   host wait.  The creation stream is ordered behind it, as for nrc_renderer_framebuffer.  A renderer on which none of these calls
 *   is made allocates and launches nothing for them.  NULL on failure.
 * nrc_renderer_set_path_aov_target: the next nrc_renderer_render_path / _render_path_timed call writes view i's AOV -- of that view's
 *   camera and, in a timed path, its in-between medium -- to d_aovs + i * h * w * 4 (device memory, n_views * h * w * 4 floats).  That
 *   call consumes the target.  A path call whose n_cameras is not n_views fails with NRC_ERR_INVALID, enqueues nothing and drops the
 *   target.  d_aovs == NULL cancels.  When the path call returns, the creation stream is ordered behind the last AOV, as it is for
 *   d_frames.  Frames, d_frames and training state are bit for bit what they are without a target.
 * nrc_renderer_export_exr_aov: nrc_renderer_export_exr with FLOAT channels A, B, G, R, Z, Zhalf, tau -- A = alpha (not the
 *   framebuffer's), Z = z_front; B, G, R the framebuffer's.  Readers of the RGBA file still find R, G, B, A.
 * nrc_test_view_aov_host (test hook): the same image computed on the CPU inside the library, by the header's plain voxel walk, for the
 *   scene as a renderer of w x h pixels would hold it (tile: as for nrc_renderer_create_tiled, or NULL); host memory, no device. */
const float* nrc_renderer_view_aov(nrc_renderer_t* r);
int nrc_renderer_set_path_aov_target(nrc_renderer_t* r, float* d_aovs, uint32_t n_views);
int nrc_renderer_export_exr_aov(nrc_renderer_t* r, const char* path);
const float* nrc_mc_renderer_view_aov(nrc_mc_renderer_t* r);
int nrc_mc_renderer_set_path_aov_target(nrc_mc_renderer_t* r, float* d_aovs, uint32_t n_views);
int nrc_mc_renderer_export_exr_aov(nrc_mc_renderer_t* r, const char* path);
int nrc_test_view_aov_host(const nrc_scene* scene, const nrc_camera* camera, uint32_t w, uint32_t h, const nrc_tile* tile, float* host_out);

/* ---------------------------------------------------------------------------------------------------------
 * Ray AOV: the view AOV's four numbers {alpha, tau, z_front, z_half} along ray segments the caller supplies -- a holdout (the medium in
 * front of an object: the camera ray up to the object's depth), the medium's shadow (the directional light's rays: a shadow map), or any
 * list of segments.  Same medium, same exact walk, same arithmetic (csrc/nrc_view_aov.hpp, view_aov_walk_range); both renderers.
 *   Record.  A ray is 8 floats {ox, oy, oz, t_min, dx, dy, dz, t_max}; its result is 4 floats.
 *   Range.   The result covers the part of the ray o + t d with t in [max(t_min, 0), t_max].  d is used as given: t is the ray parameter and
 *            the optical depth is integrated against it.  With |d| = 1, t is distance, tau the optical depth the renderers mean and
 *            z_front, z_half distances from o; the Python helpers (scene.light_view, api.camera_rays) hand out unit directions.
 *   Start.   The walk begins at t0 = max(box entry, t_min, 0) + 0, in the state of the view AOV's rule: every voxel plane with t <= t0 is
 *            behind the ray.  When t0 falls inside a non-empty voxel, z_front is exactly t0.
 *   End.     The walk ends at min(box exit, t_max).  A voxel's segment [ta, tb] counts as [ta, fminf(tb, t_max)]; the walk is done after
 *            the first trip whose far plane is at or beyond t_max, and the jump out of an empty occupancy cell is such a trip.  A segment
 *            of length 0 adds nothing.
 *   Bits.    With t_min <= 0 and t_max = +inf the result is bit for bit the whole ray's (nrc_renderer_view_aov's for a camera ray).  A
 *            ray cut at t_max = T keeps the whole ray's z_front and, wherever the cut result has a finite z_half, the whole ray's z_half
 *            (formed against the voxel's own far plane, so it may lie beyond T by the rounding of one quotient); tau accumulates
 *            identically up to the cut segment.  The plain voxel walk and the walk that jumps out of empty cells agree in every bit for
 *            every range, and so do the kernel and the host.
 *   Empty.   {0, 0, +inf, +inf} for t_max <= max(t_min, 0), a NaN in any of the eight numbers, a zero or non-finite direction, a
 *            non-finite origin, and a range that holds no medium.  The result never contains a NaN.
 * Every call below enqueues ONE launch on the stream given at creation, behind the volume rebuilds enqueued so far (set_volume,
 * set_volume_bricks, set_volume_time) and, for the view's depths, behind the view's tile mask when one is due -- where
 * nrc_renderer_view_aov puts its own.  No host wait; results are not kept (the caller's buffers may change between two calls); a renderer
 * on which none of them is made allocates and launches nothing for them.  d_rays and d_out are device memory, 16-byte aligned.
 * nrc_renderer_ray_aov: ray i of d_rays [n][8] -> d_out [n][4].  Rays are independent: a permuted list gives the permuted results.
 *   n == 0 is a no-op; a NULL pointer with n > 0 returns NRC_ERR_INVALID.
 * nrc_renderer_view_aov_to_depth: every pixel's camera ray (the view AOV's) with t_min = 0 and t_max = d_depth[pixel]; d_depth [h][w]
 *   fp32, distance along the pixel's ray -- the unit of z_front --, d_out [h][w][4]; a sharded renderer's local columns.  A depth of +inf
 *   gives nrc_renderer_view_aov's bits, a depth <= 0 or NaN the empty result.  A tile the view's mask rejects is empty whatever its depths.
 * nrc_renderer_ortho_aov: an orthographic image of w x h pixels, its size independent of the renderer's: pixel (i, j) is the whole ray
 *   from origin + su du + sv dv, su = (i + 1/2) / w, sv = (j + 1/2) / h, along dir; d_out [h][w][4].
 * nrc_renderer_set_path_aov_depths: with an AOV target set (nrc_renderer_set_path_aov_target), the next render_path call holds view i's
 *   AOV out to d_depths + i * h * w (device memory, n_views * h * w floats).  Consumed by that call like the target, and dropped with it;
 *   NULL cancels; depths without a target, or for another number of views, fail the path call with NRC_ERR_INVALID.  Frames, d_frames and
 *   training state are bit for bit what they are without it.
 * nrc_camera_rays / nrc_ortho_rays (host memory, no renderer, no device): the records {o, 0, d, +inf} of the rays the two image-shaped
 *   calls walk, [h][w][8] -- the camera's for a renderer of w x h pixels (tile: as for nrc_renderer_create_tiled, or NULL).  The
 *   image-shaped calls ARE nrc_renderer_ray_aov on these records, with t_max replaced by the depth; callers who build their own segment
 *   lists (several depth layers per pixel) start from them.
 * nrc_test_ray_aov_host (test hook): the list call on the CPU inside the library, by the header's plain voxel walk; host memory. */
typedef struct nrc_ortho_view {
    float origin[3], du[3], dv[3], dir[3];
} nrc_ortho_view;
int nrc_renderer_ray_aov(nrc_renderer_t* r, size_t n, const float* d_rays, float* d_out);
int nrc_renderer_view_aov_to_depth(nrc_renderer_t* r, const float* d_depth, float* d_out);
int nrc_renderer_ortho_aov(nrc_renderer_t* r, const nrc_ortho_view* view, uint32_t w, uint32_t h, float* d_out);
int nrc_renderer_set_path_aov_depths(nrc_renderer_t* r, const float* d_depths, uint32_t n_views);
int nrc_mc_renderer_ray_aov(nrc_mc_renderer_t* r, size_t n, const float* d_rays, float* d_out);
int nrc_mc_renderer_view_aov_to_depth(nrc_mc_renderer_t* r, const float* d_depth, float* d_out);
int nrc_mc_renderer_ortho_aov(nrc_mc_renderer_t* r, const nrc_ortho_view* view, uint32_t w, uint32_t h, float* d_out);
int nrc_mc_renderer_set_path_aov_depths(nrc_mc_renderer_t* r, const float* d_depths, uint32_t n_views);
int nrc_camera_rays(const nrc_camera* camera, uint32_t w, uint32_t h, const nrc_tile* tile, float* host_rays);
int nrc_ortho_rays(const nrc_ortho_view* view, uint32_t w, uint32_t h, float* host_rays);
int nrc_test_ray_aov_host(const nrc_scene* scene, size_t n, const float* host_rays, float* host_out);

/* ---------------------------------------------------------------------------------------------------------
 * Deep AOV: the depths at which a ray reaches given optical depths -- the transmittance FUNCTION of a pixel (a deep image) or of a light-map
 * texel (a deep shadow map), for depths that are not known when the call is made: an object can be placed inside the medium later without
 * another walk.  Same records, ranges, medium and walk as the ray AOV; both renderers; ONE walk per ray whatever the number of levels.
 *   Levels.  n_levels host floats L[0] < L[1] < .. < L[n_levels - 1], 1 <= n_levels <= 32, finite, L[0] > 0: optical depths (alpha =
 *            1 - exp(-L)).  They are read during the call; the caller may reuse the array at once.
 *   Result.  z[k] is the ray parameter at which the accumulated optical depth of the record's range reaches L[k], formed exactly as z_half
 *            is: in the non-empty voxel whose segment [ta, tb] (cut at te = fminf(tb, t_max)) takes tau to tau_new = fma(sigma, te - ta, tau),
 *            every level tau < L[k] <= tau_new gets z[k] = fminf(ta + (L[k] - tau) / sigma, tb).  A level the range never reaches is +inf.
 *            z[k] is finite exactly when the flat result's tau >= L[k] (an fp32 compare); finite depths do not decrease with k; z_front <=
 *            z[0].  With one level L = {ln 2 as fp32, 0x1.62e430p-1f} the plane is z_half bit for bit, and a level's plane does not depend
 *            on the other levels of the call.
 *   Layout.  Planar: level k of ray i is d_z[k * n + i] -- [n_levels][n], or [n_levels][h][w] for the image-shaped calls.  d_flat is NULL or
 *            receives the ray AOV's {alpha, tau, z_front, z_half} of the same records ([n][4] / [h][w][4], 16-byte aligned), with the bits
 *            the ray AOV's calls give.
 *   Empty.   An empty or degenerate record (the ray AOV's list) gives +inf in every plane and the empty flat result; never a NaN.
 * Every call enqueues ONE launch where the ray AOV's calls put theirs (behind the volume rebuilds enqueued so far and, for the camera's
 * rays, behind the view's tile mask when one is due); no host wait, nothing kept, nothing allocated; a renderer on which none of them is
 * made launches nothing for them.  NRC_ERR_INVALID, with a message and before anything is enqueued: n_levels == 0 or > 32; levels that
 * are not strictly ascending, not finite or <= 0; NULL levels or d_z; NULL d_rays with n > 0.  n == 0 is a no-op.
 * nrc_renderer_deep_ray_aov: ray i of d_rays [n][8].
 * nrc_renderer_deep_view_aov: every pixel's camera ray up to d_depth [h][w] (nrc_renderer_view_aov_to_depth's rays); d_depth NULL: whole
 *   rays.  A tile the view's mask rejects holds +inf in every plane.
 * nrc_renderer_deep_ortho_aov: the orthographic view of nrc_renderer_ortho_aov, whole rays: a deep shadow map.
 * nrc_test_deep_ray_aov_host (test hook): the list call on the CPU inside the library, by the header's plain voxel walk; host memory. */
int nrc_renderer_deep_ray_aov(nrc_renderer_t* r, size_t n, const float* d_rays, uint32_t n_levels, const float* levels, float* d_z, float* d_flat);
int nrc_renderer_deep_view_aov(nrc_renderer_t* r, const float* d_depth, uint32_t n_levels, const float* levels, float* d_z, float* d_flat);
int nrc_renderer_deep_ortho_aov(nrc_renderer_t* r, const nrc_ortho_view* view, uint32_t w, uint32_t h, uint32_t n_levels, const float* levels,
                                float* d_z, float* d_flat);
int nrc_mc_renderer_deep_ray_aov(nrc_mc_renderer_t* r, size_t n, const float* d_rays, uint32_t n_levels, const float* levels, float* d_z, float* d_flat);
int nrc_mc_renderer_deep_view_aov(nrc_mc_renderer_t* r, const float* d_depth, uint32_t n_levels, const float* levels, float* d_z, float* d_flat);
int nrc_mc_renderer_deep_ortho_aov(nrc_mc_renderer_t* r, const nrc_ortho_view* view, uint32_t w, uint32_t h, uint32_t n_levels,
                                   const float* levels, float* d_z, float* d_flat);
int nrc_test_deep_ray_aov_host(const nrc_scene* scene, size_t n, const float* host_rays, uint32_t n_levels, const float* levels, float* host_z,
                               float* host_flat);

/* ---------------------------------------------------------------------------------------------------------
 * Denoise: an edge-avoiding a-trous filter over a frame, guided by the view AOV of the same view (both renderers; every renderer call has
 * an nrc_mc_renderer_ twin).  The guide is exact and noise-free -- a function of camera and medium alone -- so the filter never smooths
 * across the medium's silhouette or a step in depth, and never touches sky.  It is a deterministic function of two images, opt-in, and
 * BIASED: it is for low frame counts and previews (DESIGN.md section 4.19 has the measured gains, the bias and where it starts to lose).
 *   Inputs.   colour c [h][w][4] fp32 RGBA (the framebuffer's layout); guide g [h][w][4] fp32 {alpha, tau, z_front, z_half} (a view AOV), of
 *             which only alpha and z_front are read; output [h][w][4].  All 16-byte aligned device memory.
 *   Params.   nrc_denoise_params: passes 1 .. 6 (default 3); sigma_alpha (0.1); sigma_depth (4.0, in the units of t); sigma_color (+inf:
 *             the term is off); color_decay (0.5), in (0, 1].  Every sigma must be > 0, +inf allowed, and large enough that 1 / sigma --
 *             for the colour term 1 / (sigma_color color_decay^(passes - 1)) -- is finite in fp32.  NaN and anything out of range:
 *             NRC_ERR_INVALID.  nrc_denoise_params_default fills the defaults.
 *   Passes.   Pass p = 0 .. passes - 1 has stride s = 1 << p, reads c_p (c_0 = c) and writes c_{p+1}; the result is c_passes.
 *   Copied.   Pixel P = (x, y) is copied bit for bit when alpha_P == 0 (sky and mask-rejected tiles, whose guide is {0, 0, +inf, +inf}:
 *             nothing is computed from their z_front) or when R, G or B of c_p(P) is not finite.
 *   Taps.     Otherwise Q = (x + i s, y + j s) for j = -2 .. 2 (outer loop), i = -2 .. 2 (inner loop), in that order, skipping a tap that
 *             lies outside the image, has alpha_Q == 0, or has a non-finite R, G or B in c_p.  For every kept tap, in fp32:
 *               k = h[i + 2] h[j + 2],  h = {1, 4, 6, 4, 1} / 16                      (exact)
 *               d = |alpha_Q - alpha_P| inv_sa
 *               d = fma(|z_front_Q - z_front_P|, inv_sz, d)
 *               d = fma(|lum_Q - lum_P|, inv_sc_p, d),   lum = fma(.114f, b, fma(.587f, g, .299f r)) of c_p
 *               wgt = k (1.0f - nrc_expm1_negf(d))                                     (csrc/nrc_math.h)
 *               acc_c = fma(wgt, c_Q - c_P, acc_c) for R, G, B;   acc_w += wgt
 *             with inv_sa = 1.0f / sigma_alpha, inv_sz = 1.0f / sigma_depth and inv_sc_p = 1.0f / (sigma_color color_decay^p), the power
 *             formed by p fp32 multiplications of sigma_color.  sigma = +inf gives an inverse, and a term, of exactly 0.
 *             out = c_P + acc_c / acc_w: the weighted mean sum(wgt c_Q) / sum(wgt), formed around the centre so that the roundings are of
 *             the size of the local contrast -- a constant colour over a constant guide comes back bit for bit.  d is not clamped: nrc_expm1_negf is exactly 1 from 17.5 on (such a tap adds nothing) and 0 for a NaN,
 *             which only a guide outside the view AOV's contract can produce (alpha != 0 beside a non-finite z_front) and which so counts
 *             as d = 0.  The centre tap has wgt = 36 / 256: acc_w is never 0.
 *   Alpha.    The output's alpha channel is the colour input's bits in every case.
 * The fp32 arithmetic is defined once, in csrc/nrc_denoise.hpp, which the kernel and the host (nrc_test_denoise_host) both run: the same
 * bits.  No in-place operation: an output that overlaps the colour, the guide or the scratch returns NRC_ERR_INVALID.
 * nrc_denoise: the free function over whole images -- what a caller with a gathered frame uses.  d_scratch: nrc_denoise_scratch_bytes
 *   bytes (0 for refused arguments).  One launch that packs the guide and one launch per pass on `stream`; no host wait.
 * nrc_renderer_denoised_frame: the current framebuffer filtered with the current view AOV (computed through nrc_renderer_view_aov's path
 *   if stale); device memory owned by the renderer, valid until it is destroyed, rewritten by the next call.  Enqueued on the renderer's
 *   streams behind the frames enqueued so far and in front of the framebuffer's next blend or clear; no host wait; the creation stream is
 *   ordered behind it, as for nrc_renderer_framebuffer.  The image and the scratch are allocated by the first call: a renderer on which it
 *   is never made allocates and launches nothing.  NULL on failure.
 * nrc_renderer_set_path_denoise_target: the next nrc_renderer_render_path / _render_path_timed call writes view i's filtered final frame
 *   to d_denoised + i * h * w * 4 (device memory, n_views * h * w * 4 floats), behind the view's last blend and in front of the next view's
 *   clear.  It needs an AOV target in the same call (nrc_renderer_set_path_aov_target): view i's guide is the caller's own d_aovs[i], so
 *   no view overwrites another's guide.  AOV depths are forbidden (the guide would be a held-out AOV).  A path call with an n_views
 *   mismatch, without an AOV target or with depths fails with NRC_ERR_INVALID, enqueues nothing and drops every target.  Consumed by that
 *   call; d_denoised == NULL cancels.  When the path call returns the creation stream is ordered behind the last filtered frame.
 *   Frames, d_frames, AOVs and training state are bit for bit what they are without the target.
 * nrc_renderer_export_exr_denoised: nrc_renderer_export_exr_aov's channels with B, G, R taken from the filtered frame.
 * A renderer that draws one rank's column strips of a sharded frame (nrc_renderer_create_tiled with x_stride > 1) refuses every renderer
 *   call above with NRC_ERR_INVALID: its local image has no pixel neighbours.  Gather the frame and the AOV and call nrc_denoise.
 * nrc_test_denoise_host (test hook): the header's arithmetic on the CPU inside the library; host memory, no device. */
typedef struct nrc_denoise_params {
    uint32_t passes;
    float sigma_alpha, sigma_depth, sigma_color, color_decay;
} nrc_denoise_params;
void nrc_denoise_params_default(nrc_denoise_params* p);
size_t nrc_denoise_scratch_bytes(uint32_t w, uint32_t h, const nrc_denoise_params* params);
int nrc_denoise(const float* d_rgba, const float* d_aov, uint32_t w, uint32_t h, const nrc_denoise_params* params, float* d_out, void* d_scratch,
                void* stream);
const float* nrc_renderer_denoised_frame(nrc_renderer_t* r, const nrc_denoise_params* params);
int nrc_renderer_set_path_denoise_target(nrc_renderer_t* r, float* d_denoised, uint32_t n_views, const nrc_denoise_params* params);
int nrc_renderer_export_exr_denoised(nrc_renderer_t* r, const char* path, const nrc_denoise_params* params);
const float* nrc_mc_renderer_denoised_frame(nrc_mc_renderer_t* r, const nrc_denoise_params* params);
int nrc_mc_renderer_set_path_denoise_target(nrc_mc_renderer_t* r, float* d_denoised, uint32_t n_views, const nrc_denoise_params* params);
int nrc_mc_renderer_export_exr_denoised(nrc_mc_renderer_t* r, const char* path, const nrc_denoise_params* params);
int nrc_test_denoise_host(const float* rgba, const float* aov, uint32_t w, uint32_t h, const nrc_denoise_params* params, float* out);

/* ---------------------------------------------------------------------------------------------------------
 * Reproject: history reuse by reprojection (both renderers; the renderer call has an nrc_mc_renderer_ twin).  The frame accumulated over
 * the views before this one is carried into the current view and blended with the current view's frames by effective frame counts, so a
 * turntable or fly-through of a few frames per view shows more samples per pixel than it renders per view.  What reprojection needs is the
 * depth of a pixel, and the view AOV has it exact and noise-free: z_half, the distance at which the camera ray reaches optical depth ln 2,
 * or z_front where the medium is thinner than that.  No motion vectors, no G-buffer.  It is a deterministic function of its images and
 * cameras, opt-in, and BIASED (DESIGN.md section 4.20 has the measured gains and the bias).
 *   Inputs.   History, all or none: colour hist_rgba [h][w][4], count hist_count [h][w] (the effective number of frames behind each pixel),
 *             the history view's AOV hist_aov [h][w][4] and its camera.  Current: colour rgba [h][w][4], the scalar frames > 0 (finite: the
 *             frames blended into it), its AOV aov [h][w][4] and its camera.  Outputs out [h][w][4], out_count [h][w].  Device memory, the
 *             images 16-byte aligned.  d_hist_rgba == NULL means no history: then all four history arguments must be NULL, out = rgba bit
 *             for bit and out_count = frames.  A NULL here and a pointer there: NRC_ERR_INVALID.
 *   Params.   nrc_reproject_params: max_history (64; > 0, finite: a cap on the frames history may count for), sigma_alpha (0.1),
 *             sigma_depth (4.0, in the units of t) -- the denoiser's defaults.  Every sigma must be > 0, +inf allowed (the term is then
 *             exactly 0), and large enough that 1 / sigma is finite in fp32.  NaN and anything out of range: NRC_ERR_INVALID.
 *   Setup.    Once per call, on the host, in double, from the history camera's fp32 inv_proj_view m and pos:  A_k = m[k] - pos_k m[3],
 *             B_k = m[4 + k] - pos_k m[7],  C_k = m[12 + k] - pos_k m[15]  (k = 0, 1, 2) -- a history pixel's ray direction is
 *             ~ sx A + sy B + C.  N = [A B C]^-1, rounded to fp32.  A determinant of 0 or a non-finite N: NRC_ERR_INVALID.
 *   Pixel.    P = (x, y), in fp32, in this order (csrc/nrc_reproject.hpp is the one statement; its head is this list's fine print):
 *             1. alpha_P == 0, a non-finite R, G or B of rgba(P), or no history: out = rgba(P) bit for bit, out_count = frames.
 *             2. z = finite(z_half_P) ? z_half_P : z_front_P.
 *             3. the view AOV's camera ray of the pixel (u = x (1.0f / w), v = y (1.0f / h): no half-pixel offset); X = fma(z, rd, ro).
 *             4. D = X - pos_hist;  q_k = fma(N[3k + 2], D_2, fma(N[3k + 1], D_1, N[3k] D_0));  sx = q_0 / q_2, sy = q_1 / q_2;
 *                ww = fma(m[7], sy, fma(m[3], sx, m[15])); the pixel passes through unless q_2 ww > 0 (X in front of the history
 *                camera);  dist = |D|.
 *             5. fx = ((sx + 1) 0.5) w, fy likewise with h; the pixel passes through unless -1 <= fx < w and -1 <= fy < h;
 *                x0 = floor(fx), tx = fx - x0, and likewise for y.
 *             6. the taps Q = (x0 + i, y0 + j), j = 0, 1 outside, i = 0, 1 inside, skipping a tap outside the image, with alpha_Q == 0,
 *                or with a non-finite R, G or B in hist_rgba.  z_Q as in 2.  b = (i ? tx : 1 - tx) (j ? ty : 1 - ty);
 *                  d = |alpha_Q - alpha_P| inv_sa;  d = fma(|z_Q - dist|, inv_sz, d);  wgt = b (1.0f - nrc_expm1_negf(d))
 *                  acc_c = fma(wgt, c_Q - c_P, acc_c) for R, G, B;  acc_w += wgt;  acc_n = fma(wgt, n_Q, acc_n)
 *                The depth term is the disocclusion test: the history pixel must have seen the medium at the distance X has from the
 *                history camera.  The mean is formed around the centre: a constant colour comes back bit for bit.
 *             7. acc_w == 0: the pixel passes through.  Otherwise n_h = min(acc_n, max_history), a = n_h / (n_h + frames),
 *                out = fma(a, acc_c / acc_w, c_P) for R, G, B, out_count = n_h + frames.
 *             acc_n is not normalised: the bilinear weights and exp(-d) shrink it, so poorly matched history counts for little, without a
 *             threshold.  The rule is continuous in (fx, fy).
 *   Alpha.    The output's alpha channel is the current colour's bits in every case.
 * The fp32 arithmetic is defined once, in csrc/nrc_reproject.hpp, which the kernel and the host (nrc_test_reproject_host) both run: the same
 * bits.  No in-place operation: an output that overlaps any input, or the other output, returns NRC_ERR_INVALID before anything is enqueued.
 * nrc_reproject: the free function over whole images; one launch on `stream`, no host wait, nothing allocated.
 * nrc_renderer_set_path_reproject_target: view i of the next nrc_renderer_render_path / _render_path_timed call writes
 *     accum[i], counts[i] = reproject(history: accum[i - 1], counts[i - 1], aovs[i - 1], cameras[i - 1];
 *                                     current: the view's final framebuffer, frames_per_camera, aovs[i], cameras[i])
 *   to d_accum + i * h * w * 4 and d_counts + i * h * w (device memory for n_views views); view 0 has no history.  It is enqueued behind
 *   the view's last blend and in front of the next view's clear, behind view i - 1's reprojection.  It needs an AOV target in the same
 *   call (nrc_renderer_set_path_aov_target): the caller's d_aovs[i - 1] and d_aovs[i] are the guides.  A path call without an AOV target,
 *   with AOV depths, with another n_views, with frames_per_camera == 0 or with a singular camera fails with NRC_ERR_INVALID, enqueues
 *   nothing and drops every target.  Consumed by that call; d_accum == NULL cancels.  With a denoise target in the same call view i's
 *   filter reads accum[i] instead of the framebuffer, behind the reprojection: accumulate, then filter.  With a timed path the medium
 *   may change between views: history is validated by the guides alone, whose depth and alpha then differ where the medium moved.  When the
 *   path call returns the creation stream is ordered behind the last reprojection.  The renderer allocates nothing for this: every buffer
 *   is the caller's.  Frames, d_frames, AOVs and training state are bit for bit what they are without the target.
 * A renderer that draws one rank's column strips of a sharded frame refuses the renderer call with NRC_ERR_INVALID.
 * nrc_test_reproject_host (test hook): the header's arithmetic on the CPU inside the library; host memory, no device. */
typedef struct nrc_reproject_params {
    float max_history, sigma_alpha, sigma_depth;
} nrc_reproject_params;
void nrc_reproject_params_default(nrc_reproject_params* p);
int nrc_reproject(const float* d_hist_rgba, const float* d_hist_count, const float* d_hist_aov, const nrc_camera* hist_camera, const float* d_rgba,
                  float frames, const float* d_aov, const nrc_camera* camera, uint32_t w, uint32_t h, const nrc_reproject_params* params, float* d_out,
                  float* d_out_count, void* stream);
int nrc_test_reproject_host(const float* hist_rgba, const float* hist_count, const float* hist_aov, const nrc_camera* hist_camera, const float* rgba,
                            float frames, const float* aov, const nrc_camera* camera, uint32_t w, uint32_t h, const nrc_reproject_params* params,
                            float* out, float* out_count);
int nrc_renderer_set_path_reproject_target(nrc_renderer_t* r, float* d_accum, float* d_counts, uint32_t n_views, const nrc_reproject_params* params);
int nrc_mc_renderer_set_path_reproject_target(nrc_mc_renderer_t* r, float* d_accum, float* d_counts, uint32_t n_views,
                                              const nrc_reproject_params* params);

/* THE environment switch of the library: NRC_DEBUG="name[=value],..." -- diagnostic and test switches only, none changes a result
 * (the list and what each does: csrc/nrc_common.hpp, debug_switch).
 * diagnostics (read when the library first allocates): NRC_DEBUG=poison_alloc fills every device allocation with 0xFF
 * bytes at creation; NRC_DEBUG=guard_alloc puts 4 KiB canaries around every allocation.  nrc_debug_check_guards returns -1 when the
 * guard mode is off, otherwise the number of allocations whose canaries were overwritten (0 = clean) and, in message, the first.
 * nrc_debug_live_allocations (always on): device allocations the library holds right now, nrc_image_create's included -- what it was
 * before an object was created is what it is again after the object is destroyed, or after its creation failed. */
int nrc_debug_check_guards(char* message, size_t message_bytes);
int nrc_debug_live_allocations(void);

/* ---------------------------------------------------------------------------------------------------------
 * Test hooks (bit-parity of the math spec and RNG against the oracle; device pointers) */
int nrc_test_math(int fn, const float* d_a, const float* d_b, uint32_t n, float* d_out, float* d_out2, void* stream);
int nrc_test_rng(float u, float v, const float frame_random[4], uint32_t n, float* d_out, void* stream);
/* the capped-state side of the empty-space skip, as the renderers use it: selects from the process-wide free-flight table (2^23 floats, one
 * per RNG state: the optical distance of 128 free flights) the states whose entry does not exceed lambda.  d_count_and_list: 9 words, the
 * count and the first eight states found (any order); d_bits: 2^18 + 2 words, bit (m & 31) of word (m >> 5) set for every selected state m
 * (the two words behind them are the slack a renderer's own buffer has: never written).  d_table_out: NULL, or 2^23 floats that receive
 * a copy of the table.  Everything is enqueued on `stream`; no product path calls this. */
int nrc_test_flight_select(float lambda, float* d_table_out, uint32_t* d_count_and_list, uint32_t* d_bits, void* stream);

#ifdef __cplusplus
}
#endif
#endif
