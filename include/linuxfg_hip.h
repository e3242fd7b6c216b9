/*
 * linuxfg_hip.h -- C-ABI of the MI355X-native linux-fg hot path
 *                  (upscale -> motion -> interpolate).
 *
 * This is the drop-in boundary.  The reference (xXJSONDeruloXx/linux-fg) has no plugin
 * or FFI layer: its boundary is the C++ class surface VulkanContext / FrameManager /
 * Scaler.  Everything those classes do on the hot path through
 * Vulkan is provided here through plain C: opaque context, POD frame descriptor, plain
 * pointers and sizes, int return codes.  The C++ mirror of the reference classes in
 * linux-fg_amd/host/ and the ctypes binding in linux-fg_amd/capi.py call nothing else.
 *
 * Conventions
 *   - every fallible call returns 0 on success, a negative lfg_status otherwise, and
 *     latches a message readable with lfg_last_error() (the reference returns bool and
 *     latches Logger::GetLastError, src/logger.hpp:33-41); nothing throws across this ABI;
 *   - a context is bound to ONE GPU and ONE HIP stream and is not thread-safe (the
 *     reference is single-threaded, one VkQueue: src/vulkan_context.cpp:130-151);
 *   - compute calls ENQUEUE on the context's stream and return; lfg_sync() waits
 *     (the reference waits with vkQueueWaitIdle after every submit, src/scaler.cpp:393);
 *   - frames are row-major, `pitch` bytes per row, RGBA8 = 4 bytes per pixel in memory
 *     order R,G,B,A (channel order is irrelevant to the kernels: all four are treated alike);
 *   - there is no CPU fallback: without a usable GPU lfg_context_create() fails.
 *
 * All citations are file:line under the reference checkout.
 */
#ifndef LINUXFG_HIP_H
#define LINUXFG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LFG_ABI_VERSION 1

typedef enum lfg_status {
    LFG_OK = 0,
    LFG_ERR_INVALID = -1,     /* bad argument (null, size mismatch, unsupported parameter) */
    LFG_ERR_DEVICE = -2,      /* HIP runtime error; text in lfg_last_error() */
    LFG_ERR_NOMEM = -3,
    LFG_ERR_UNSUPPORTED = -4
} lfg_status;

typedef enum lfg_format {
    /* VK_FORMAT_R8G8B8A8_UNORM, the only colour format the reference creates
     * (src/frame_manager.hpp:15). 4 bytes per pixel. */
    LFG_FORMAT_RGBA8_UNORM = 0,
    /* Motion vectors, two signed bytes per pixel (x, y), whole pixels in [-127,127].
     * The reference declares the MV image rgba32f (shaders/motion.comp:7) and stores
     * vec4(best, 0, 1) (:56); best is always integer-valued for the integer search radii
     * the host pushes (src/frame_manager.cpp:333), so two int8 hold it losslessly at 1/8
     * of the bytes.  lfg_mv_export_rgba32f() reproduces the reference's image verbatim. */
    LFG_FORMAT_MV_S8X2 = 1,
    /* Motion vectors in quarter pixels, four bytes per pixel: int16 x in the low half, int16 y in the high half.  Rows are
     * 4-byte aligned and the pitch is a multiple of 4.  A frame may hold any 16-bit values; every reader clamps each component
     * to [-508, 508] (= 4 * 127) before use.  Written by lfg_motion_subpel, read by lfg_interpolate_compensated_subpel.  No
     * reference counterpart. */
    LFG_FORMAT_MV_S16X2_Q2 = 2
} lfg_format;

/* Replaces `struct Frame` {VkImage, VkDeviceMemory, VkImageView, width, height, format}
 * (src/frame_manager.hpp:9-16): a device pointer plus geometry.  Caller-owned POD. */
typedef struct lfg_frame {
    void    *data;      /* device memory; NULL = empty frame (VK_NULL_HANDLE) */
    uint32_t width;
    uint32_t height;
    uint32_t pitch;     /* bytes per row, >= width * bytes-per-pixel and <= 0x7fffffff: every call returns LFG_ERR_INVALID
                         * for a larger one before anything is enqueued or allocated (the frame kernels take it as an int).
                         * lfg_mask.pitch and the lfg_nv12 pitches have no such limit. */
    uint32_t format;    /* lfg_format */
    uint32_t owned;     /* 1: allocated by lfg_frame_create and freed by lfg_frame_destroy */
    uint32_t reserved;
} lfg_frame;

typedef struct lfg_context lfg_context;
typedef struct lfg_ring lfg_ring;

/* Kernel stages, for lfg_profile_get(). */
typedef enum lfg_stage {
    LFG_STAGE_SCALE = 0,
    LFG_STAGE_MOTION = 1,
    LFG_STAGE_INTERPOLATE = 2,
    LFG_STAGE_COUNT = 3
} lfg_stage;

/* ---------------------------------------------------------------- library / context */

int         lfg_abi_version(void);
/* Number of HIP devices visible to this process (0 if none); does not create a context. */
int         lfg_device_count(void);

/* Replaces VulkanContext::Initialize (src/vulkan_context.cpp:3-23: instance, physical
 * device pick :88-105, logical device + one compute queue :117-151).  device_ordinal < 0
 * picks device 0 (the reference prefers a discrete GPU, else index 0).  The context owns
 * one HIP stream (the compute queue) unless lfg_context_set_stream() adopts another. */
int         lfg_context_create(int device_ordinal, lfg_context **out_ctx);
/* Replaces VulkanContext::Cleanup / FrameManager::Cleanup / Scaler::Cleanup.  NULL is a no-op. */
void        lfg_context_destroy(lfg_context *ctx);
/* Adopt an externally owned hipStream_t (a stream the caller created, e.g. a PyTorch side
 * stream's handle) as the selected lane's compute queue: the calls made on that lane run on it,
 * so the caller's events and collectives order against these kernels.  NULL -- handle 0 --
 * restores the lane's own stream and adopts nothing: HIP's null stream, which is handle 0 and is
 * PyTorch's DEFAULT stream, cannot be adopted.  The stream stays the caller's: shrinking the lanes
 * and destroying the context wait for it and never destroy it.  lfg_context_get_stream returns
 * the stream the selected lane's calls run on, its own or the adopted one. */
int         lfg_context_set_stream(lfg_context *ctx, void *hip_stream);
void       *lfg_context_get_stream(lfg_context *ctx);
int         lfg_context_device(const lfg_context *ctx);
/* vkQueueWaitIdle (src/scaler.cpp:393, src/frame_manager.cpp:194): every lane of the context. */
int         lfg_sync(lfg_context *ctx);

/* Lanes: several frames in flight on one GPU.  The reference has one queue and waits for it after every
 * submission (src/scaler.cpp:389-393, src/frame_manager.cpp:190-194); here a frame's last long motion units leave
 * most CUs idle for a third of its time, and the next frame's scale, hints and first units can run there.  A lane
 * is a stream plus the temporaries and the motion workspace (0.9 GB at 4K, 1.0 GB for the one lane of a context without lanes: lfg_motion_workspace_size) of the calls made while it is selected;
 * frames are plain device memory and may be used from any lane -- the caller orders producers and consumers:
 *   lfg_lanes(ctx, n)       1 <= n <= LFG_MAX_LANES lanes (lane 0 is the context's own stream); shrinking waits
 *                           for the lanes that go and frees what they own
 *   lfg_lane_select(ctx, j) the calls that follow enqueue on lane j
 *   lfg_lane_mark(ctx)      remember "here" on the selected lane
 *   lfg_lane_wait(ctx, i)   the selected lane's later work waits until lane i has reached its last mark: the newest
 *                           lfg_lane_mark made on lane i before this call, not the end of lane i -- what lane i was given
 *                           after that mark is not waited for; before lane i's first mark, and for i the selected lane
 *                           itself, the call orders nothing
 *   lfg_lane_sync(ctx)      the HOST waits for the selected lane alone (a frame's buffers are free again; lfg_sync waits for
 *                           every lane) -- what vkQueueWaitIdle after each submission (src/scaler.cpp:389-393) becomes when
 *                           n frames are in flight: wait for frame k before frame k + n goes onto its lane
 * e.g. frame k on lane k % 2:  select; scale(curr_k); mark; wait(other lane: scale(curr_k-1)); motion; interpolate.
 * lfg_context_set_stream applies to the selected lane. */
#define LFG_MAX_LANES 4
int         lfg_lanes(lfg_context *ctx, int count);
int         lfg_lane_count(const lfg_context *ctx);
int         lfg_lane_current(const lfg_context *ctx);
int         lfg_lane_select(lfg_context *ctx, int lane);
int         lfg_lane_mark(lfg_context *ctx);
int         lfg_lane_wait(lfg_context *ctx, int other);
int         lfg_lane_sync(lfg_context *ctx);
/* Logger::GetLastError (src/logger.hpp:38).  ctx == NULL reads the creation-time error. */
const char *lfg_last_error(const lfg_context *ctx);

/* ---------------------------------------------------------------- frames */

/* FrameManager::CreateFrame (src/frame_manager.cpp:30-69): device-local storage for a
 * width x height image; pitch is tight (width * bpp rounded up to 16 bytes is NOT applied:
 * rows are tightly packed so a frame is one contiguous upload). */
int  lfg_frame_create(lfg_context *ctx, uint32_t width, uint32_t height, uint32_t format, lfg_frame *out);
/* FrameManager::DestroyFrame (src/frame_manager.cpp:71-81): idempotent, NULL-safe. */
void lfg_frame_destroy(lfg_context *ctx, lfg_frame *frame);
/* Describe caller-owned device memory (e.g. a torch tensor) as a frame; never freed here.  LFG_ERR_INVALID for a pitch below
 * width * bytes-per-pixel (compared in 64 bits) or above 0x7fffffff (lfg_frame.pitch). */
int  lfg_frame_wrap(void *device_ptr, uint32_t width, uint32_t height, uint32_t pitch, uint32_t format,
                    lfg_frame *out);
/* FrameManager::CopyFrameData (src/frame_manager.cpp:83-145): same-size check, then a
 * device-to-device copy on the stream. */
int  lfg_frame_copy(lfg_context *ctx, const lfg_frame *src, lfg_frame *dst);

/* FrameManager::CreateStagingBuffer / DestroyStagingBuffer (src/frame_manager.cpp:199-214):
 * host-visible memory the device can DMA from; here pinned host memory. */
int  lfg_staging_create(lfg_context *ctx, size_t bytes, void **out_host_ptr);
void lfg_staging_destroy(lfg_context *ctx, void *host_ptr);

/* Upload = WindowCapture::CopyToStagingBuffer (src/window_capture.cpp:472-568): `bytes` must be
 * >= width*height*bpp (the reference's size check, :478-481); rows tightly packed.  Download =
 * the readback in Scaler::ProcessFrame (src/scaler.cpp:479-536).  Both are asynchronous on the
 * stream when `host` is pinned (lfg_staging_create / ring memory); call lfg_sync() before
 * touching the host bytes. */
int  lfg_frame_upload(lfg_context *ctx, lfg_frame *dst, const void *host, size_t bytes);
int  lfg_frame_download(lfg_context *ctx, const lfg_frame *src, void *host, size_t bytes);

/* Pinned-host frame ring: replaces the per-frame staging alloc/free of the reference
 * (src/window_capture.cpp:474-487,564; src/scaler.cpp:480-487,614).  `slots` buffers of
 * `slot_bytes` each; acquire blocks until the slot's last transfer has completed. */
int  lfg_ring_create(lfg_context *ctx, uint32_t slots, size_t slot_bytes, lfg_ring **out_ring);
void lfg_ring_destroy(lfg_ring *ring);
int  lfg_ring_acquire(lfg_ring *ring, void **out_host_ptr, uint32_t *out_slot);
/* Upload slot -> frame (or download frame -> slot) asynchronously and mark the slot busy
 * until that transfer finishes.  Transfers run on the ring's own stream, next to the kernels, and
 * are ordered against the lane SELECTED AT THE CALL, no other: an upload is ordered after everything
 * enqueued on that lane so far and before everything enqueued on it later; a download is ordered
 * after everything enqueued on that lane so far only -- later kernels do not wait for it.  Work on
 * another lane that reads or writes the frame is the caller's to order (lfg_lane_mark / lfg_lane_wait). */
int  lfg_ring_upload(lfg_ring *ring, uint32_t slot, lfg_frame *dst);
int  lfg_ring_download(lfg_ring *ring, uint32_t slot, const lfg_frame *src);
/* Block the host until the slot's last transfer has finished (the vkQueueWaitIdle before the
 * reference maps its staging buffer, src/scaler.cpp:532-536), then the slot's pixels may be read. */
int  lfg_ring_wait(lfg_ring *ring, uint32_t slot);
/* Make kernels enqueued on the selected lane from now on wait (on the device, not the host) for the slot's last transfer:
 * call it before overwriting a frame whose download into `slot` may still be running. */
int  lfg_ring_fence_slot(lfg_ring *ring, uint32_t slot);

/* ---------------------------------------------------------------- the three stages */

/* shaders/scale.comp as dispatched by Scaler::ScaleFrame (src/scaler.cpp:260-395):
 * Lanczos-3 resample of `in` to `out`'s size; push constants inputSize/outputSize are taken
 * from the frames (src/scaler.cpp:348-351).  Any sizes; out == 2 x in takes the LDS-tiled path. */
int  lfg_scale(lfg_context *ctx, const lfg_frame *in, lfg_frame *out);
/* Which scale kernel the context's last lfg_scale or lfg_interpolate_scale launched: 0 the generic kernel (any sizes; also
 * 2x when the pitch or alignment rules fail, or a frame spans 2 GiB or more), 1 the exact-2x kernel, 2 the fused
 * interpolate -> 2x scale kernel; -1 before any scale.  Tests and reporting only. */
int  lfg_scale_last_kernel(const lfg_context *ctx);

/* shaders/motion.comp as dispatched by FrameManager::InterpolateFrames
 * (src/frame_manager.cpp:325-344): per-pixel full-search block match of `curr` against `prev`.
 * `mv` is an LFG_FORMAT_MV_S8X2 frame of the same size.  The reference pushes blockSize = 8,
 * searchRadius = 16.0f (:332-333); other values are accepted when searchRadius is a whole
 * number in [0,127] and 1 <= blockSize <= 64. */
int  lfg_motion(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *mv,
                int block_size, float search_radius);

/* How lfg_motion evaluates blockSize 8 / searchRadius 16.  Both modes return bit-identical motion
 * vectors for every input; they differ in run time only.
 *   LFG_MOTION_PREFILTERED (default): a cheap value that provably brackets every candidate's cost (integer
 *       squared distances, pairwise-tree sums; within 3.6e-5 relative of the shader's sequential fp32 sum
 *       for any data) selects the few candidates that can still be the minimum; a single survivor is the
 *       answer, several get the literal 64-term chain.  Tiles where many candidates tie at one non-zero cost
 *       fall back to the exact kernel, so such content costs what LFG_MOTION_EXACT_ONLY costs (plus the filter).
 *   LFG_MOTION_EXACT_ONLY: the literal chain for every (pixel, candidate); content-independent time. */
typedef enum lfg_motion_mode { LFG_MOTION_PREFILTERED = 0, LFG_MOTION_EXACT_ONLY = 1 } lfg_motion_mode;
int  lfg_set_motion_mode(lfg_context *ctx, int mode);
/* After a prefiltered lfg_motion: number of 64x64 tiles, how many of them fell back to the exact kernel,
 * and the mean number of candidates recorded per pixel in the others (synchronises; reporting only). */
int  lfg_motion_last_stats(lfg_context *ctx, uint32_t *out_tiles, uint32_t *out_fallback_tiles,
                           double *out_mean_recorded);
/* After a prefiltered lfg_motion: how many 16-row segments of its 56 x 64 work tiles the prefilter left to the resolve
 * kernel, and how many the frame has; every open segment is listed exactly once (synchronises; reporting and tests only).
 * No reference counterpart: motion.comp (shaders/motion.comp:27-52) has one pass and no work lists. */
int  lfg_motion_open_segments(lfg_context *ctx, uint32_t *out_open, uint32_t *out_segments);
/* After a prefiltered lfg_motion: how many entries of the run-time queue its work units asked for -- a unit that holds a whole
 * tile hands a segment without a match over to the workgroups that run out of units, one entry per four parts of the segment --
 * and how many entries the queue is laid out for; what does not fit is searched in place.  Zero at frame sizes whose tiles are
 * all shared between several units (synchronises; reporting and tests only).  No reference counterpart, as above. */
int  lfg_motion_hand_over_stats(lfg_context *ctx, uint32_t *out_entries_asked, uint32_t *out_entries_room);
/* With frames in flight (lfg_lanes >= 2) a call whose content suits it sends its whole interior tiles through a lean kernel
 * before the general one (same vectors; the choice goes by the lane's previous call).  After an lfg_motion: whether the selected
 * lane's last call did (1/0), how many tiles are listed for that kernel at this frame size, and in how many it left work to the
 * general kernel (synchronises; reporting and tests only).  No reference counterpart (shaders/motion.comp:27-52 is one pass). */
int  lfg_motion_lean_stats(lfg_context *ctx, int *out_used, uint32_t *out_tiles, uint32_t *out_tiles_left);
/* The strips a frame's motion exposes along its edges -- sixteen pixel columns, eight rows: pixels without any match -- are
 * searched by a kernel of their own before the general one (same vectors).  After an lfg_motion: how many pixel rows had their
 * left or right band decided that way and how many pixel columns their top or bottom band (synchronises; reporting and tests
 * only).  No reference counterpart (shaders/motion.comp:27-52 treats every pixel alike). */
int  lfg_motion_strip_stats(lfg_context *ctx, uint32_t *out_rows, uint32_t *out_columns);
/* The persistent motion kernel exists in two variants with identical results: the default, and one whose lattice walks go by sums
 * of absolute differences first where a match costs a few hundred to a thousand -- sensor noise of +-3 levels and more at a
 * 1080p input (4K, three frames in flight: +15 % at +-3, +27 % at +-4 .. +-12; -3 % at +-2 and below, which is why it is not the
 * only one).  With frames in flight the lane's previous call decides (half its sample blocks matched with a SAD of 310 - 2,200);
 * LFG_TIER_FORCE=0|1 at context creation overrides.  Returns the variant the context's last lfg_motion launched (0 / 1). */
int  lfg_motion_last_variant(const lfg_context *ctx);
/* With frames in flight four launch decisions of an lfg_motion go by what the lane's PREVIOUS finished call found (its
 * verdict word, stored into pinned host memory by that call's last launch): the lean kernel and the plan that goes with it,
 * the size of the persistent grid and the variant of its kernel (counted together), the size of the second pass.  A wrong guess changes no result, only the call's duration.
 * Counters since the context was created, over all lanes: calls whose own verdict has been read back, and how many of them
 * had been launched on a guess that this verdict contradicts, per decision (does not synchronise; reporting only).
 * No reference counterpart: one queue, one dispatch per stage (src/frame_manager.cpp:342-366). */
int  lfg_motion_prediction_stats(const lfg_context *ctx, uint64_t *out_verdicts, uint64_t *out_lean_wrong,
                                 uint64_t *out_grid_wrong, uint64_t *out_second_pass_wrong);
/* Bytes of device memory the prefiltered lfg_motion keeps for frames of this size (allocated on the first such call, kept
 * until the size changes or the context goes; one per lane).  No reference counterpart -- the reference's motion pass keeps
 * nothing between its two images (src/frame_manager.cpp:262-300); a host budgets lanes with it.  Needs no GPU work.
 * The figure is for the context's CURRENT lane count (the work-unit plan of a context with frames in flight differs from
 * that of a context without, see lfg_motion_plan): call it after lfg_lanes(). */
int  lfg_motion_workspace_size(lfg_context *ctx, uint32_t width, uint32_t height, uint64_t *out_bytes);
/* The work-unit plan the prefiltered lfg_motion uses on this context: *out_rim_split = parts of the candidate order a
 * segment on the image's rim is searched in -- 4 with frames in flight (lfg_lanes >= 2: the sum of the units' times counts),
 * 48 = four, and eight for the segments at the top and bottom border, when one frame runs at a time (the longest unit counts);
 * LFG_MOTION_RIM_SPLIT=4|8|48 in the environment at context creation overrides -- and *out_workgroups = the persistent
 * workgroups the device holds for its prefilter launch (0 before the first call; with frames in flight a call launches 5/8 of
 * them when the lane's previous call found most of its sample blocks matched and another lane is busy: room for their kernels).  The plan changes only inside lfg_lanes(); the first lfg_motion
 * after such a change re-plans (it waits for the lane's stream once).  Reporting only; either pointer may be NULL. */
int  lfg_motion_plan(const lfg_context *ctx, int *out_rim_split, int *out_workgroups);

/* Coarse-to-fine (pyramid) block matcher, opt-in, next to the full search.  No reference counterpart: the reference has one
 * +-16 full search (shaders/motion.comp:27-47).  Writes the same LFG_FORMAT_MV_S8X2 vectors -- 8 x 8 block p + [-4,3]^2,
 * curr texels outside the image skipped, prev outside the image read as 0, prev(q + v) ~ curr(q) -- so every consumer of
 * lfg_motion's output takes them unchanged.  Integer arithmetic only:
 *   - levels 1 .. L of both frames: W_k = ceil(W_{k-1} / 2) (likewise H), each channel of P_k(x,y) the rounded mean
 *     (sum + 2) >> 2 of P_{k-1} at (2x + i, 2y + j), i, j in {0,1}, coordinates clamped to the level;
 *   - cost C_k(p, v) = sum over the block's texels q inside level k of sum_c |curr_k(q)_c - prev_k(q + v)_c|;
 *   - the minimum of the key (C, vx^2 + vy^2, vy, vx) wins (not affected by lfg_set_semantics);
 *   - level L: v in [-coarse_radius, coarse_radius]^2; level k < L: c + [-refine_radius, refine_radius]^2 and (0,0), with
 *     c = 2 * v_{k+1}(x / 2, y / 2); mv = v_0.
 * 1 <= levels <= 4, 1 <= coarse_radius <= 32, 1 <= refine_radius <= 4 and coarse_radius * 2^levels + refine_radius *
 * (2^levels - 1) <= 127 (the longest vector); otherwise LFG_ERR_UNSUPPORTED before anything is enqueued.  The range is
 * that bound: (2, 16, 2) reaches +-70 px.  Each call costs the same on any content.  Frames as lfg_motion takes them (RGBA8
 * 4-byte aligned, any size).  Enqueued on the selected lane; keeps, per lane, device memory of
 * 10 * sum over k = 1 .. levels of W_k * H_k bytes (plus up to 256 bytes of alignment per array): about 26 MB at 4K with
 * (2, 16, 2).  Timed under LFG_STAGE_MOTION. */
int  lfg_motion_pyramid(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, lfg_frame *mv,
                        int levels, int coarse_radius, int refine_radius);
/* The motion estimator of lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   LFG_ESTIMATOR_FULL_SEARCH (default): lfg_motion(8, 16), the reference's;
 *   LFG_ESTIMATOR_PYRAMID: lfg_motion_pyramid(2, 16, 2) into the lane's temporary, then the interpolate stage
 *       (lfg_set_fused_motion_interpolate does not apply).  Under the reference semantics a vector of 2 px or more moves both
 *       of lfg_interpolate's samples out of the image; LFG_SEMANTICS_INTENDED keeps them inside, but with the shader's signs,
 *       which are backwards for these vectors (see LFG_SEMANTICS_INTENDED).  Content that moves wants
 *       lfg_set_interpolator(LFG_INTERPOLATOR_COMPENSATED). */
typedef enum lfg_motion_estimator { LFG_ESTIMATOR_FULL_SEARCH = 0, LFG_ESTIMATOR_PYRAMID = 1 } lfg_motion_estimator;
int  lfg_set_motion_estimator(lfg_context *ctx, int estimator);

/* Which arithmetic lfg_motion and lfg_interpolate follow.  No reference counterpart: SURVEY.md 8(f) rank 4.
 *   LFG_SEMANTICS_REFERENCE (default, the parity contract): the shaders as written -- equal block-match costs
 *       resolve to the first candidate in scan order, so flat areas report (-16,-16) (shaders/motion.comp:27-28,49;
 *       F6), and the pixel-unit motion vector is added to normalised uv unscaled (shaders/interpolate.comp:17,34-35; F5).
 *   LFG_SEMANTICS_INTENDED (opt-in): equal costs resolve to the shortest vector (then scan order), so flat areas
 *       report (0,0); interpolate divides the vector by the image size before adding it to uv, so it displaces
 *       by pixels.  Everything else (costs, sampling, signs, rounding) is unchanged; the oracle has the same switch.
 *       The signs stay the shader's (interpolate.comp:34-35): prev is read at g - v t and curr at g + v (1 - t), while the
 *       vectors (prev(q + v) ~ curr(q)) put the content at g + v t in prev and g - v (1 - t) in curr.  So for moving content
 *       the two samples land 2 |v| apart and neither is the content at g: every generated frame of a pan is a double image.
 *       This mode stays as it is (pinned by the tests); lfg_interpolate_compensated is the interpolation that moves content
 *       to where it is at time t, and it wants this mode for its motion stage (flat areas then report (0,0)). */
typedef enum lfg_semantics { LFG_SEMANTICS_REFERENCE = 0, LFG_SEMANTICS_INTENDED = 1 } lfg_semantics;
int  lfg_set_semantics(lfg_context *ctx, int semantics);

/* shaders/interpolate.comp (src/frame_manager.cpp:351-366): MV-displaced bilinear fetch of prev
 * and curr, blended by `factor`.  Literal reference semantics (MV in pixels added to normalised
 * UV). */
int  lfg_interpolate(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                     lfg_frame *out, float factor);

/* FrameManager::InterpolateFrames(previous, current, output, factor)
 * (src/frame_manager.cpp:216-372): motion (blockSize 8, searchRadius 16) then interpolate, with
 * the motion-vector image as a context-owned temporary (the reference creates and destroys it
 * per call, :226-230,369; here it persists between calls and is invisible to the caller). */
int  lfg_interpolate_frames(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                            lfg_frame *out, float factor);

/* Several generated frames per pair -- the 60 -> 240 fps cadence of BASELINE config 5 (t = 1/4, 1/2, 3/4) -- from
 * ONE pass over prev, curr and the motion vectors (the vectors and both sources are read once
 * per pair instead of once per factor).  No reference counterpart beyond the single `factor` of
 * FrameManager::InterpolateFrames (src/frame_manager.cpp:216) and ScalerConfig::interpolationFactor
 * (src/scaler.hpp:17).  outs[i] receives the frame for factors[i]; every frame is identical, byte for byte, to
 * lfg_interpolate(ctx, prev, curr, mv, outs[i], factors[i]).  1 <= count <= LFG_MAX_FACTORS; the outputs must
 * not alias each other or an input. */
#define LFG_MAX_FACTORS 16
int  lfg_interpolate_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                           lfg_frame *const *outs, const float *factors, uint32_t count);
/* lfg_interpolate_frames in the north-star ORDER (the reference dispatches motion and then
 * interpolate on the same grid, src/frame_manager.cpp:342-366, the second reading what the first wrote): with 1, the
 * motion kernels (blockSize 8, searchRadius 16 paths) write the generated frame from each vector at the moment it is
 * decided -- the same per-pixel function the interpolate kernel is made of, so the bytes are identical -- the interpolate
 * dispatch is gone and the motion-vector temporary is never written.  Default 0: the two stages (measured: DESIGN.md
 * section 4.4).  Also set by LFG_FUSED_MOTION_INTERPOLATE=1 in the environment at context creation.  lfg_interpolate_frames_multi
 * always runs the two stages. */
int  lfg_set_fused_motion_interpolate(lfg_context *ctx, int enabled);

/* lfg_interpolate_frames for several factors: motion (blockSize 8, searchRadius 16) ONCE, then
 * lfg_interpolate_multi with the context-owned motion-vector temporary. */
int  lfg_interpolate_frames_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                                  lfg_frame *const *outs, const float *factors, uint32_t count);

/* Motion-compensated interpolation, opt-in, next to the shader's path.  No reference counterpart (the reference samples at
 * g -+ mv(g), shaders/interpolate.comp:34-35).  The vectors are projected forward to time t and both frames are fetched along
 * the projected vectors; pixels that nothing lands on are occlusions.  Always in pixels and with the vectors' own signs: it
 * does not depend on lfg_set_semantics.  All float arithmetic is fp32 without contraction.
 *   Inputs: prev, curr RGBA8 and mv LFG_FORMAT_MV_S8X2 (as lfg_motion / lfg_motion_pyramid write it; any byte values), all
 *   W x H; factor t finite in [0, 1], s = 1.0f - t; 0 <= match_sad <= 1020.
 *   Match gate: q with v = mv(q) is matched when sum over c of |curr(q)_c - prev(q + v)_c| <= match_sad, prev outside the
 *   image read as 0.  An unmatched pixel's content is not in prev: its vector does not project.
 *   Projection, every matched q: dx = (int)floorf((float)v.x * s + 0.5f), dy likewise, d = q + (dx, dy); outside the image
 *   dropped, otherwise atomicMin of the key ((65535 - (vx^2 + vy^2)) << 16) | ((vy + 128) << 8) | (vx + 128) into K(d), K
 *   starting at 0xFFFFFFFF (a hole).  The longest vector wins, then the smallest vy, then the smallest vx (without depth the
 *   larger motion is taken for the foreground); the order is total, so the result does not depend on scheduling.
 *   Sampling at d with the vector u decoded from K(d): P = ((float)d.x + 0.5f) + (float)u.x * t, C = ((float)d.x + 0.5f) -
 *   (float)u.x * s, y likewise, each fetched with the bilinear clamp-to-edge rule of lfg_interpolate (same floor, weights and
 *   sum order) in pixel units: u' = P.x - 0.5f.  A sample is inside when 0 <= x <= W and 0 <= y <= H.  Output: mix(Pv, Cv, t)
 *   when both are inside or neither is, else the inside one; stored as lfg_interpolate stores (clamp, x 255, half to even).
 *   Holes (K(d) = 0xFFFFFFFF): walk from d in each of the four axis directions, k = 1 .. 16, stopping at the image edge, and
 *   keep each direction's first non-hole pixel; u = the smallest (|v|^2, vy, vx) of the kept vectors (the background-most),
 *   (0, 0) if none.  P and C as above, and c = (clamp((int)floorf(C.x), 0, W - 1), likewise y): c unmatched -> Cv alone
 *   (content revealed in curr); c matched with mv(c) != u -> Pv alone (content covered in curr); else as a projected pixel.
 *   Hence t = 1 gives curr exactly for any vectors and match_sad, and a uniform even vector at t = 0.5 gives prev shifted by
 *   -v / 2 on the interior.
 * Frames: 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4), 2-byte aligned mv; the outputs must not overlap each
 * other or any input.  Any violation, and a NaN, infinite or out-of-range factor or match_sad, returns LFG_ERR_INVALID before
 * anything is enqueued.  Keeps, per lane, device memory of 4 * W * H bytes (33 MB at 4K), grown on demand.  Enqueued on the
 * selected lane (clear K, project, interpolate per factor); timed under LFG_STAGE_INTERPOLATE.  _multi: 1 <= count <=
 * LFG_MAX_FACTORS, outs[i] for factors[i], each identical to the single call. */
int  lfg_interpolate_compensated(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                 lfg_frame *out, float factor, int match_sad);
int  lfg_interpolate_compensated_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                       lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad);
/* The interpolation of lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   LFG_INTERPOLATOR_SHADER (default): lfg_interpolate[_multi], the reference's shader; every path as before;
 *   LFG_INTERPOLATOR_COMPENSATED: the selected estimator (lfg_set_motion_estimator) into the lane's temporary, then
 *       lfg_interpolate_compensated[_multi] with match_sad (lfg_set_fused_motion_interpolate does not apply).  Use it with
 *       LFG_SEMANTICS_INTENDED for the motion stage: under the reference tie order flat areas report (-16,-16).
 * 0 <= match_sad <= 1020 (the default is 48); otherwise, or for an unknown interpolator, LFG_ERR_INVALID and no change. */
typedef enum lfg_interpolator { LFG_INTERPOLATOR_SHADER = 0, LFG_INTERPOLATOR_COMPENSATED = 1 } lfg_interpolator;
int  lfg_set_interpolator(lfg_context *ctx, int interpolator, int match_sad);

/* Static-overlay protection for the compensated interpolation, opt-in.  No reference counterpart.  A crosshair, a line of text
 * or a health bar does not move while the scene behind it pans; in a stroke pixel's 8 x 8 block the moving background outvotes
 * the stroke, and the compensated interpolation then moves the overlay's pixels with the background.
 * A mask says which pixels are static; the masked call keeps those where they are and keeps them out of what moves past them.
 *   Mask: one byte per pixel in caller-owned device memory; a non-zero byte means static.  Like lfg_nv12 it is no lfg_format:
 *   it is described by an lfg_mask.  pitch >= width, any alignment.
 *   lfg_static_mask: out(q) = 255 when the sum over the four channels c of |prev(q)_c - curr(q)_c| <= tolerance, else 0;
 *   0 <= tolerance <= 1020.  prev, curr RGBA8 of the mask's W x H, 4-byte aligned rows.  Only the W bytes of each mask row
 *   are written, never the row padding; the mask overlaps neither frame.  Any violation or a NULL pointer returns
 *   LFG_ERR_INVALID before anything is enqueued.  One launch on the selected lane; it keeps no device memory and is outside
 *   the stage timers.  A host that knows its own UI passes its own mask instead.
 *   lfg_interpolate_compensated_masked[_multi]: lfg_interpolate_compensated[_multi]'s arguments and `mask` after `mv`; its
 *   definition word for word, with S(q) = (mask(q) != 0) and these five changes:
 *   1. Projection: every q with S(q) also does atomicMin(K(q), 0).  Key 0 is the static marker: no vector's key is 0, since
 *      65535 - |v|^2 >= 32767.  q then goes through the match gate and projects its own vector exactly as before (the overlap
 *      of a flat moving object with itself is static by any such test, and must keep projecting).  A static location
 *      therefore always ends as 0, whatever lands on it.
 *   2. Sampling at d with K(d) = 0: mix(unorm(prev(d)_c), unorm(curr(d)_c), t) per channel from the two texels directly;
 *      the same mix and store rule, no positions.
 *   3. Hole walk: a pixel whose key is 0 is passed over like a hole and the walk goes on: an overlay is not the surface
 *      behind it.
 *   4. Fetch rule, for every d with K(d) != 0, holes included, before the hole's revealed / covered test and before the
 *      inside test: p = (clamp((int)floorf(P.x), 0, W - 1), likewise y), and c likewise from C.  S(p) && !S(c) -> Cv alone (the
 *      content is hidden under the overlay in prev); S(c) && !S(p) -> Pv alone; otherwise the sample proceeds as before.
 *   5. Hence an all-zero mask gives lfg_interpolate_compensated's bytes for any input.
 * Frames: lfg_interpolate_compensated's rules; the mask has the frames' W x H and overlaps no output; it is only read.  A
 * NULL mask or mask->data, a size mismatch or pitch < width returns LFG_ERR_INVALID before anything is enqueued.  The same
 * launches, lane, device memory and stage timer as lfg_interpolate_compensated. */
typedef struct lfg_mask { void *data; uint32_t width, height, pitch; } lfg_mask;   /* caller-owned device memory */
int  lfg_static_mask(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, int tolerance, const lfg_mask *out);
int  lfg_interpolate_compensated_masked(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                        const lfg_mask *mask, lfg_frame *out, float factor, int match_sad);
int  lfg_interpolate_compensated_masked_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                              const lfg_mask *mask, lfg_frame *const *outs, const float *factors, uint32_t count,
                                              int match_sad);
/* Static protection in lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   tolerance = -1 (default): off; every path as before;
 *   0 .. 1020, with LFG_INTERPOLATOR_COMPENSATED selected: the vectors as before (the selected estimator, then the refinement if
 *       it is on), lfg_static_mask(prev, curr, tolerance) once per pair into a per-lane temporary (W x H bytes, grown on
 *       demand, freed with the lane), then lfg_interpolate_compensated_masked[_multi] in lfg_interpolate_compensated[_multi]'s
 *       place; cut detection runs around it as before;
 *   with LFG_INTERPOLATOR_SHADER selected the setting is stored and has no effect.
 * Any other value: LFG_ERR_INVALID and no change. */
int  lfg_set_static_protection(lfg_context *ctx, int tolerance);

/* Motion-compensated extrapolation, opt-in: the frame at time 1 + a, AHEAD of the newest frame, predicted from the motion just
 * measured.  No reference counterpart (the reference only generates frames between two real ones).  Every interpolated frame
 * holds the newest real frame back by a source-frame interval; an extrapolated one does not: the real frame is presented as it
 * arrives and the generated ones follow it.  curr's content is projected forward along its vectors and curr
 * alone is fetched along the projected vectors.  Always in pixels and with the vectors' own signs: it does not depend on
 * lfg_set_semantics.  All float arithmetic is fp32 without contraction.
 *   Inputs: prev, curr RGBA8 and mv LFG_FORMAT_MV_S8X2 (any byte values), all W x H; `ahead` a finite in [0, 1], prev being at
 *   time 0 and curr at time 1; 0 <= match_sad <= 1020.
 *   Match gate: lfg_interpolate_compensated's, word for word: q with v = mv(q) is matched when sum over c of |curr(q)_c -
 *   prev(q + v)_c| <= match_sad, prev outside the image read as 0.  An unmatched pixel's motion is unknown: it does not project.
 *   Projection: content at q in curr came from q + v, so it moves by -v per interval.  Every matched q: dx = (int)floorf(0.5f -
 *   (float)v.x * a), dy likewise, d = q + (dx, dy); outside the image dropped, otherwise atomicMin of
 *   lfg_interpolate_compensated's key ((65535 - (vx^2 + vy^2)) << 16) | ((vy + 128) << 8) | (vx + 128) into K(d), K starting at
 *   0xFFFFFFFF (a hole): the longest vector wins, then the smallest vy, then the smallest vx.
 *   Sampling at d with the vector u decoded from K(d): C = ((float)d.x + 0.5f) + (float)u.x * a, y likewise; the output is curr
 *   fetched at C with the bilinear clamp-to-edge rule of lfg_interpolate_compensated (same floor, weights and sum order, in
 *   pixel units), stored as it stores.  prev is never sampled: only the match gate reads it.
 *   Holes (K(d) = 0xFFFFFFFF): walk from d in the directions +x, -x, +y, -y in that order, k = 1 .. 16, stopping at the image
 *   edge, and keep each direction's first non-hole pixel n.  Of the kept pixels the one with the smallest (|v|^2, vy, vx) (the
 *   background-most) is the donor, on an equal triple the earlier direction's; u is its vector and n its position.  If no
 *   direction kept one, u = (0, 0) and there is no donor.  C as above and c = (clamp((int)floorf(C.x), 0, W - 1), likewise y).
 *   If there is a donor, c is matched and mv(c) != u, curr shows the foreground at c and the surface behind it is visible in
 *   neither frame: then C := ((float)n.x + 0.5f) + (float)u.x * a, y likewise -- the background's edge is stretched over what
 *   the foreground vacates instead of leaving a copy of the foreground behind it.  In every other case C stays.  The output is
 *   curr fetched at C.
 *   Hence a = 0 gives curr exactly for any vectors and match_sad; a uniform vector v that matches everywhere gives out(d) =
 *   curr(d + v) at a = 1 and, for even v, curr(d + v / 2) at a = 0.5, both at every d whose source (d + v, d + v / 2) lies inside
 *   the image.
 * Frames and errors: lfg_interpolate_compensated's rules (4-byte aligned RGBA8 rows of any pitch that is a multiple of 4, 2-byte
 * aligned mv, outputs overlapping neither each other nor an input).  Any violation, and a NaN, infinite or out-of-range `ahead`
 * or match_sad, returns LFG_ERR_INVALID before anything is enqueued.  Uses the lane's key image of lfg_interpolate_compensated
 * (4 * W * H bytes, grown on demand) and keeps no other device memory.  Enqueued on the selected lane (clear K, project, sample
 * per factor); timed under LFG_STAGE_INTERPOLATE.  _multi: 1 <= count <= LFG_MAX_FACTORS, outs[i] for aheads[i], each identical
 * to the single call.  Not built: a masked (overlay-protected) extrapolation, a projection shared between factors, a > 1. */
int  lfg_extrapolate_compensated(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                 lfg_frame *out, float ahead, int match_sad);
int  lfg_extrapolate_compensated_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                       lfg_frame *const *outs, const float *aheads, uint32_t count, int match_sad);
/* What lfg_interpolate_frames and lfg_interpolate_frames_multi generate (nothing else):
 *   LFG_GENERATION_INTERPOLATE (default): frames between prev and curr; every path as before;
 *   LFG_GENERATION_EXTRAPOLATE, with LFG_INTERPOLATOR_COMPENSATED selected: the vectors as before (the selected estimator, then
 *       the refinement if it is on), then lfg_extrapolate_compensated[_multi] in the compensated interpolator's place, each
 *       factors[i] read as an `ahead`.  With cut detection on, lfg_pair_match and the record run as before and lfg_cut_fallback
 *       is enqueued with every factor passed as 1.0f: a cut gives curr, the newest frame repeated, for every output.
 *       lfg_set_static_protection has no effect on extrapolated frames (a masked extrapolation is not built), and
 *       lfg_set_fused_motion_interpolate does not apply;
 *   with LFG_INTERPOLATOR_SHADER selected the setting is stored and has no effect.
 * Any other value: LFG_ERR_INVALID and no change. */
typedef enum lfg_generation { LFG_GENERATION_INTERPOLATE = 0, LFG_GENERATION_EXTRAPOLATE = 1 } lfg_generation;
int  lfg_set_generation(lfg_context *ctx, int generation);

/* Bidirectional motion-compensated interpolation, opt-in: lfg_interpolate_compensated with a second vector field, measured the
 * other way, that checks the first and projects from prev's grid as well.  No reference counterpart.  Always in pixels and with
 * the vectors' own signs: it does not depend on lfg_set_semantics.  All float arithmetic is fp32 without contraction; the
 * predicates are integer arithmetic.
 *   Fields: fwd is LFG_FORMAT_MV_S8X2 on curr's grid, as lfg_motion(prev, curr) writes it: prev(q + f) ~ curr(q).  bwd is on
 *   prev's grid, as lfg_motion(curr, prev) writes it: curr(p + b) ~ prev(p).  Any byte values; components in [-128, 127].
 *   confirmed_f(q), f = fwd(q): lfg_interpolate_compensated's match gate holds (sum over c of |curr(q)_c - prev(q + f)_c| <=
 *   match_sad, prev outside the image read as 0); p = q + f lies inside the image; and with b = bwd(p), |f.x + b.x| + |f.y + b.y|
 *   <= tolerance.
 *   confirmed_b(p), b = bwd(p): the mirror image: sum over c of |prev(p)_c - curr(p + b)_c| <= match_sad, curr outside read as
 *   0; q = p + b lies inside; |b.x + fwd(q).x| + |b.y + fwd(q).y| <= tolerance; and neither component of b is -128 (its negation
 *   does not fit the vector word).
 * lfg_motion_consistency is the vector half of the two predicates on its own, with no frames and no gate: out(q) = 255 when r = q
 * + a(q) lies inside the image and |a(q).x + b(r).x| + |a(q).y + b(r).y| <= tolerance, otherwise 0; called with (fwd, bwd) it
 * answers for curr's grid, with (bwd, fwd) for prev's: the occlusion map of a pair.  a, b MV_S8X2 of one size, 2-byte aligned; 0
 * <= tolerance <= 64; out of the fields' size with pitch >= width, overlapping neither field (lfg_static_mask's rules); only
 * the W bytes of each row are written.  One launch on the selected lane, no device memory kept, outside the stage timers.
 *
 * lfg_interpolate_compensated_bidirectional is lfg_interpolate_compensated's definition word for word, with these changes:
 *   Forward projection: every q with confirmed_f(q) (not merely matched) projects as there: d = q + (floorf((float)f.x * s +
 *   0.5f), likewise y), s = 1.0f - t; outside the image dropped, otherwise atomicMin of the key of (f.x, f.y) into K(d).
 *   Backward projection, into the same K: every p with confirmed_b(p) projects to d = p + (floorf((float)b.x * t + 0.5f),
 *   likewise y); outside dropped, otherwise atomicMin of the key of (-b.x, -b.y): the content of p moves by +b per interval, so
 *   in fwd's convention it carries u = -b.  Near t = 0, where the forward displacement is nearly the whole vector and its
 *   rounding leaves cracks between regions, the backward one is small, and the other way round.  The key order is total, so K
 *   does not depend on scheduling or on which projection ran first.
 *   Sampling at a non-hole: unchanged (u decoded from K(d), P, C, the taps, the inside rule, the mix, the store).
 *   Holes: the walk, its 16-pixel reach, its direction order and the choice of u are unchanged.  With c = clamp(floor(C)) and p
 *   = clamp(floor(P)): Cbad = confirmed_f(c) && fwd(c) != u (curr shows other, confirmed content there); Pbad = confirmed_b(p)
 *   && -bwd(p) != u (prev does).  Cbad && !Pbad: the prev sample alone (the content is covered in curr).  Pbad && !Cbad: the curr
 *   sample alone (revealed in curr).  In every other case the pixel goes on as a projected pixel: the inside rule, then the mix.
 *   Hence t = 1 gives curr exactly and t = 0 gives prev exactly, for any fields, match_sad and tolerance: at t = 0 every
 *   confirmed_b pixel projects onto itself, so a hole at d is not confirmed_b, Pbad is false, P = d and mixf(x, y, 0) is x; at t
 *   = 1 the same holds with the roles exchanged.  (lfg_interpolate_compensated promises only the second.)
 * Frames and errors: lfg_interpolate_compensated's rules, bwd held to fwd's (MV_S8X2 of the frames' size, 2-byte aligned, no
 * output overlapping it); 0 <= tolerance <= 64.  Any violation returns LFG_ERR_INVALID before anything is enqueued, with a
 * message latched.  Uses the lane's key image of lfg_interpolate_compensated and keeps no other device memory.  Enqueued on the
 * selected lane (clear K, project forward, project backward, sample, per factor); timed under LFG_STAGE_INTERPOLATE.  _multi: 1
 * <= count <= LFG_MAX_FACTORS, outs[i] for factors[i], each identical to the single call.  Not built: a masked
 * (overlay-protected) variant, an extrapolating variant, both fields estimated in one pass over the pair. */
int  lfg_motion_consistency(lfg_context *ctx, const lfg_frame *a, const lfg_frame *b, int tolerance, const lfg_mask *out);
int  lfg_interpolate_compensated_bidirectional(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *fwd,
                                               const lfg_frame *bwd, lfg_frame *out, float factor, int match_sad, int tolerance);
int  lfg_interpolate_compensated_bidirectional_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr,
                                                     const lfg_frame *fwd, const lfg_frame *bwd, lfg_frame *const *outs,
                                                     const float *factors, uint32_t count, int match_sad, int tolerance);
/* The bidirectional route of lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else).  -1 (default): off, every
 * path enqueues what it did.  0 .. 64 takes effect when LFG_INTERPOLATOR_COMPENSATED and LFG_GENERATION_INTERPOLATE are selected
 * and static protection is off: the selected estimator runs twice, (prev, curr) into the lane's vector temporary as before and
 * (curr, prev) into a further temporary of the lane, made on demand and freed with the lane; with lfg_set_vector_refinement on,
 * lfg_motion_refine runs on each, (prev, curr, fwd) and (curr, prev, bwd); cut detection runs on fwd as before; then
 * lfg_interpolate_compensated_bidirectional[_multi] runs with this tolerance in the compensated interpolator's place.  This
 * doubles the motion stage, the dominant cost: about 4.5 ms more per 4K pair with the pyramid.
 * The setting is stored and has no effect
 *   with LFG_INTERPOLATOR_SHADER selected;
 *   with LFG_GENERATION_EXTRAPOLATE selected (an extrapolating variant is not built);
 *   with lfg_set_static_protection on (a masked bidirectional route is not built: the masked interpolation runs as before).
 * Any other value: LFG_ERR_INVALID and no change. */
int  lfg_set_bidirectional(lfg_context *ctx, int tolerance);

/* Hole-fill reach beyond 16 px, opt-in: the fill plane.  No reference counterpart.  The hole walk of the three interpolating
 * calls above stops after 16 pixels and then fills with (0, 0); vectors of up to 127 px open holes wider than 32 px, whose
 * middle then shows doubled or misplaced background.  The fill plane gives every pixel its fill key
 * from two scan passes over K whose cost does not depend on how deep a hole is.  Integer arithmetic only.
 *   fill(x, y; reach, pass_static): in each of the directions +x, -x, +y, -y take the nearest pixel at distance 1 .. reach
 *   inside the image whose word in K is a donor.  A word is a donor if it is not the hole word 0xFFFFFFFF; with pass_static it
 *   must also not be the static word 0.  Of the donors found, at most four, the result is the smallest walk-order key
 *   ((vx^2 + vy^2) << 16) | ((vy + 128) << 8) | (vx + 128) -- the stored key with its high half replaced by 65535 minus it.
 *   If no direction has a donor the result is the hole word, which the sampling kernels read as the vector (0, 0).  The pixel
 *   itself is never its own donor, and the plane is defined at every pixel, holes or not.  At reach 16, and at every hole, this
 *   is the hole walk of lfg_interpolate_compensated (pass_static = 0) and of lfg_interpolate_compensated_masked (1), exactly.
 * lfg_hole_fill_plane: the two passes alone.  keys and plane are RGBA8 frames used as one 32-bit word per pixel, pitch
 * honoured, as lfg_frame_diff uses a frame for its record: the same size, 4-byte aligned (data and pitch), not overlapping;
 * 1 <= reach <= LFG_HOLE_REACH_MAX (twice the longest vector the word holds); pass_static 0 or 1.  Any violation or a NULL
 * pointer returns LFG_ERR_INVALID before anything is enqueued.  Two launches on the selected lane (row pass, column pass); keys
 * is only read; keeps no device memory; outside the stage timers.
 * lfg_set_hole_reach: -1 (default): off; every path enqueues and allocates what it did.  1 .. LFG_HOLE_REACH_MAX:
 * lfg_interpolate_compensated[_multi], lfg_interpolate_compensated_masked[_multi] (pass_static = 1) and
 * lfg_interpolate_compensated_bidirectional[_multi] -- called directly or by lfg_interpolate_frames[_multi] -- run, per factor,
 * clear K, project, fill plane, and a sampling kernel that takes a hole's vector from the plane: their definitions word for
 * word with "k = 1 .. 16" read as "k = 1 .. reach".  The plane is one more per-lane buffer of 4 * W * H bytes, grown on
 * demand and freed with the lane.  Any other value: LFG_ERR_INVALID and no change.  The shader interpolator ignores the
 * setting, and so does extrapolation (lfg_extrapolate_compensated[_multi], LFG_GENERATION_EXTRAPOLATE): its walk keeps the
 * step count for the donor and is another algorithm, which stays at 16. */
#define LFG_HOLE_REACH_MAX 255
int  lfg_hole_fill_plane(lfg_context *ctx, const lfg_frame *keys, int reach, int pass_static, lfg_frame *plane);
int  lfg_set_hole_reach(lfg_context *ctx, int reach);

/* Per-pixel vector refinement, opt-in, between motion estimation and interpolation.  No reference counterpart.  Both
 * estimators give each pixel the vector of the 8 x 8 block around it, so near a moving edge a band of up to ~4 px takes the
 * other side's vector; this picks, for each pixel, the nearby vector that fits a small window around that pixel best.
 * Integer arithmetic only; it does not depend on lfg_set_semantics.
 *   Inputs: prev, curr RGBA8 and mv_in, mv_out LFG_FORMAT_MV_S8X2, all W x H; mv_in may hold any byte values;
 *   0 <= radius <= 2.
 *   Candidates of pixel q: mv_in(q + o) for o = (0, 0) and o = (a s, b s), a, b in {-1, 0, 1}, (a, b) != (0, 0), s in {4, 8}:
 *   17 positions.  A position outside the image gives no candidate; mv_in(q) always is one.
 *   Cost of candidate v at q: the sum over texels r of the (2 radius + 1)^2 window centred on q, and over the four channels,
 *   of |curr(r)_c - prev(r + v)_c|; texels r outside the image are skipped, prev outside the image reads as 0 (the
 *   conventions of lfg_motion_pyramid's cost and of lfg_interpolate_compensated's match gate).
 *   mv_out(q) = the candidate with the smallest key (cost, vx^2 + vy^2, vy, vx), lfg_motion_pyramid's tie order.  The order
 *   is total, so neither the order of evaluation nor any tiling changes a result.
 * Hence: where all 17 candidates are equal (a uniform field, such as any pan) mv_out = mv_in, and every output vector is one
 * of its pixel's candidates.
 * Frames: 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4), 2-byte aligned mv; mv_out must not overlap any input
 * (every output depends on its neighbours' inputs: the call cannot run in place).  Any violation, and a radius outside
 * [0, 2], returns LFG_ERR_INVALID before anything is enqueued.  One launch on the selected lane; keeps no device memory;
 * timed under LFG_STAGE_MOTION. */
int  lfg_motion_refine(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv_in,
                       lfg_frame *mv_out, int radius);
/* Refinement in lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   radius = -1 (default): off; every path as before;
 *   radius = 0 .. 2: the selected estimator (lfg_set_motion_estimator) into the lane's temporary, lfg_motion_refine with this
 *       radius into a second per-lane temporary (W x H MV_S8X2, made on demand, freed by lfg_context_destroy), then the
 *       selected interpolator (lfg_set_interpolator) on the refined vectors; lfg_set_fused_motion_interpolate does not apply.
 * Any other radius: LFG_ERR_INVALID and no change. */
int  lfg_set_vector_refinement(lfg_context *ctx, int radius);

/* Half-resolution motion, opt-in.  No reference counterpart.  Motion estimation is the cost of a generated frame; both
 * estimators take frames of any size, so the field can be estimated on frames of half the size and carried to full size.
 * lfg_frame_halve makes the half-size frame and lfg_motion_expand the full-size field.  Integer arithmetic only; neither
 * depends on lfg_set_semantics.
 *
 * lfg_frame_halve: lfg_motion_pyramid's level rule as a call.  in RGBA8 W x H, out RGBA8 ceil(W / 2) x ceil(H / 2); each channel
 * of out(x, y) is the rounded mean (sum + 2) >> 2 of in at (2x + i, 2y + j), i, j in {0, 1}, coordinates clamped to in.
 * Frames: 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4), W, H >= 1, out overlapping no byte of in.  Any
 * violation, a NULL pointer, a wrong format or a wrong out size returns LFG_ERR_INVALID before anything is enqueued.  One
 * launch on the selected lane; keeps no device memory; timed under LFG_STAGE_MOTION. */
int  lfg_frame_halve(lfg_context *ctx, const lfg_frame *in, lfg_frame *out);
/* lfg_motion_expand: a W x H field from a ceil(W / 2) x ceil(H / 2) one, the choice steered by the full-resolution frames.
 *   Inputs: prev, curr RGBA8 and mv_out LFG_FORMAT_MV_S8X2, all W x H; mv_low MV_S8X2 of exactly ceil(W / 2) x ceil(H / 2), any
 *   byte values; 0 <= radius <= 2.
 *   dbl(v) = (clamp(2 v.x, -127, 127), clamp(2 v.y, -127, 127)).
 *   Cost of vector v at q: lfg_motion_refine's, word for word -- the sum over texels r of the (2 radius + 1)^2 window centred
 *   on q, and over the four channels, of |curr(r)_c - prev(r + v)_c|; texels r outside the image are skipped, prev outside the
 *   image reads as 0.  The smallest key (cost, vx^2 + vy^2, vy, vx) wins: lfg_motion_refine's total order.
 *   Step 1, the coarse neighbour: the candidates of q = (x, y) are dbl(mv_low(n)) for n = (x >> 1, y >> 1) + (a, b), a, b in
 *   {-1, 0, 1}.  A position n outside mv_low gives no candidate; the centre always is one.  w = the candidate with the smallest
 *   key.
 *   Step 2, the parity that doubling cannot express: the candidates are (clamp(w.x + dx, -127, 127), clamp(w.y + dy, -127,
 *   127)) for dx, dy in {-1, 0, 1}, w among them.  mv_out(q) = the one with the smallest key.
 * Hence: the order is total, so neither the order of evaluation nor any tiling changes a result; a uniform mv_low of v gives,
 * at every pixel, the best of dbl(v) + [-1, 1]^2; every output component lies in [-127, 127].
 * Frames: lfg_motion_refine's rules -- 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4), 2-byte aligned vector
 * frames -- and mv_out must not overlap any input.  Any violation, a wrong mv_low size and a radius outside [0, 2] returns
 * LFG_ERR_INVALID before anything is enqueued.  One launch on the selected lane; keeps no device memory; timed under
 * LFG_STAGE_MOTION.  Not built: other ratios than 2; an expansion fused into lfg_motion_refine or into the projection of the
 * compensated interpolators. */
int  lfg_motion_expand(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv_low,
                       lfg_frame *mv_out, int radius);
/* Half-resolution motion in lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   radius = -1 (default): off; every path enqueues and allocates what it did;
 *   radius = 0 .. 2: wherever those calls run the selected estimator -- for both directions of lfg_set_bidirectional -- they
 *       halve both frames into per-lane temporaries (lfg_frame_halve), run the estimator on the halves into a per-lane
 *       half-size vector frame -- LFG_ESTIMATOR_FULL_SEARCH: lfg_motion(8, 16); LFG_ESTIMATOR_PYRAMID: lfg_motion_pyramid(1, 16,
 *       2), which with the expansion reaches 2 (16 * 2 + 2) + 1 = 69 px -- and run lfg_motion_expand with this radius into the
 *       vector temporary the estimator wrote before.  The temporaries are made on demand, follow a change of size and are
 *       freed with the lane.  Everything downstream takes the field unchanged: refinement, cut detection, static protection,
 *       every interpolator and generation mode.  lfg_set_fused_motion_interpolate does not apply.
 * Any other radius: LFG_ERR_INVALID and no change.  Measured cost and quality: DESIGN.md section 4.18. */
int  lfg_set_half_resolution_motion(lfg_context *ctx, int radius);

/* Quarter-pixel vectors, opt-in.  No reference counterpart.  Every other vector in the library is a whole number of pixels;
 * content that moves by 2.5 px per frame then fails the compensated interpolator's match gate where nothing is wrong, and the
 * two fetches of a projected pixel land half a pixel apart.  lfg_motion_subpel refines an integer field to quarter pixels and
 * lfg_interpolate_compensated_subpel is the compensated interpolation that carries the fraction.
 *
 * lfg_motion_subpel: mvq_out(q) = the quarter-pixel vector near 4 mv_in(q) that fits q's window best.  Integer arithmetic
 * only; it does not depend on lfg_set_semantics.
 *   Inputs: prev, curr RGBA8, mv_in LFG_FORMAT_MV_S8X2 and mvq_out LFG_FORMAT_MV_S16X2_Q2, all W x H; 0 <= radius <= 2.
 *   v = mv_in(q), a byte of -128 read as -127.
 *   The fractional sample prevq(r, w) of a quarter-pixel vector w: i = (w.x >> 2, w.y >> 2) (arithmetic shift: the floor),
 *   f = (w.x & 3, w.y & 3), T00 = prev(r + i), T10 = prev(r + i + (1, 0)), T01 = prev(r + i + (0, 1)), T11 = prev(r + i + (1, 1)),
 *   a texel outside the image read as 0 in all channels; per channel
 *       ((4 - fx)(4 - fy) T00 + fx (4 - fy) T10 + (4 - fx) fy T01 + fx fy T11 + 8) >> 4.
 *   With f = (0, 0) this is prev(r + i) exactly.
 *   Cost of w at q: the sum over texels r of the (2 radius + 1)^2 window centred on q, and over the four channels, of
 *   |curr(r)_c - prevq(r, w)_c|; texels r outside the image are skipped (lfg_motion_refine's conventions).
 *   Order: with d = w - 4v the smallest key (cost, dx^2 + dy^2, dy, dx) wins.  The integer vector wins every tie -- a fraction
 *   has to earn its place with a strictly lower cost -- and the order is total, so neither the order of evaluation nor any
 *   tiling changes a result.
 *   Stage 1, half pixel: the candidates 4v + (2a, 2b), a, b in {-1, 0, 1}; the winner is h.
 *   Stage 2, quarter pixel: the candidates h + (a, b), a, b in {-1, 0, 1}; the winner is mvq_out(q).
 *   A candidate with a component outside [-508, 508] is dropped; 4v is always in range.
 * Hence: every output lies within 3 quarter pixels (Chebyshev distance) of 4v; where the windows are flat the output is
 * 4 mv_in; all texels needed lie in the (2 radius + 3)^2 block of prev around q + v.
 * Frames: lfg_motion_refine's rules -- 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4), mv_in 2-byte aligned,
 * mvq_out 4-byte aligned with a pitch that is a multiple of 4 -- and mvq_out must not overlap any input.  Any violation, a
 * NULL pointer, a wrong format or size and a radius outside [0, 2] returns LFG_ERR_INVALID before anything is enqueued.  One
 * launch on the selected lane; keeps no device memory; timed under LFG_STAGE_MOTION. */
int  lfg_motion_subpel(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv_in,
                       lfg_frame *mvq_out, int radius);
/* lfg_interpolate_compensated_subpel[_multi]: lfg_interpolate_compensated[_multi] with mvq (LFG_FORMAT_MV_S16X2_Q2, any
 * 16-bit values) in mv's place.  The definition is lfg_interpolate_compensated's word for word, with five changes:
 *   Gate: q is matched when sum over c of |curr(q)_c - prevq(q, w)_c| <= match_sad, w = mvq(q) clamped to [-508, 508].
 *   Projection: d = q + (dx, dy), dx = (int)floorf(((float)w.x * 0.25f) * s + 0.5f), s = 1 - t, dy likewise; a landing outside
 *   the image is dropped.
 *   Key order: where several pixels land on one destination the largest wx^2 + wy^2 wins, then the smallest wy, then the
 *   smallest wx (20 + 10 + 10 bits: the key image K holds 64 bits per pixel, all ones where nothing landed).
 *   Sampling: P.x = ((float)d.x + 0.5f) + ((float)u.x * 0.25f) * t, C.x = ((float)d.x + 0.5f) - ((float)u.x * 0.25f) * s, y
 *   likewise; the same bilinear fetch, inside rule, blend and store.
 *   Holes: the same four 16 px walks, each direction keeping its first non-hole; u is the smallest (|w|^2, wy, wx) of the kept
 *   vectors, (0, 0) if none; c as in lfg_interpolate_compensated; c unmatched under the fractional gate: Cv alone; c matched
 *   with mvq(c) != u (clamped): Pv alone; otherwise as a projected pixel.
 * Hence: with mvq = 4 mv (components in [-127, 127]) the output equals lfg_interpolate_compensated(mv) byte for byte, for
 * every input, factor and match_sad; t = 1 gives curr exactly.
 * Frames and checks: lfg_interpolate_compensated[_multi]'s, with mvq 4-byte aligned and its pitch a multiple of 4.  The lane
 * keeps the route's key image, 8 W H bytes, grown on demand and freed with the lane; _multi repeats the single call per
 * factor with one K.  Timed under LFG_STAGE_INTERPOLATE.
 * Not built, on purpose: masked (static protection), bidirectional, extrapolating and fill-plane (lfg_set_hole_reach)
 * variants of this route. */
int  lfg_interpolate_compensated_subpel(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mvq,
                                        lfg_frame *out, float factor, int match_sad);
int  lfg_interpolate_compensated_subpel_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mvq,
                                              lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad);
/* Quarter-pixel vectors in lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   radius = -1 (default): off; every path enqueues and allocates what it did;
 *   radius = 0 .. 2: exactly where those calls would run lfg_interpolate_compensated[_multi] with the 16 px walk -- the
 *       compensated interpolator, LFG_GENERATION_INTERPOLATE, and lfg_set_bidirectional, lfg_set_static_protection and
 *       lfg_set_hole_reach all off -- the final integer field (after half-resolution expansion and refinement) goes through
 *       lfg_motion_subpel with this radius into a per-lane MV_S16X2_Q2 temporary (made on demand, follows a change of size,
 *       freed with the lane), and lfg_interpolate_compensated_subpel[_multi] runs in the compensated call's place.
 * Under every other setting it has no effect.  Cut detection and everything else keep reading the integer field.
 * Any other radius: LFG_ERR_INVALID and no change.  Measured cost and quality: DESIGN.md section 4.20. */
int  lfg_set_subpixel_vectors(lfg_context *ctx, int radius);

/* Bicubic sampling in the compensated routes, opt-in.  No reference counterpart.  lfg_interpolate_compensated and
 * lfg_interpolate_compensated_subpel fetch prev and curr with the 2 x 2 bilinear rule, a low-pass: a generated frame at a half-
 * or quarter-pixel position is softer than the real frames on either side of it.  LFG_SAMPLING_BICUBIC replaces that fetch, and
 * nothing else, with a 4 x 4 Catmull-Rom fetch defined in integers.
 *
 * The table Wt[phi][k], phi = 0 .. 63, k = 0 .. 3: Catmull-Rom at f = phi / 64 in 14-bit fixed point, from exact integers.
 *   n0 = -4096 phi + 128 phi^2 - phi^3,  n1 = 524288 - 320 phi^2 + 3 phi^3,  n2 = 4096 phi + 256 phi^2 - 3 phi^3,
 *   n3 = -64 phi^2 + phi^3 (they sum to 524288 = 2 * 64^3);  Wt[phi][k] = (n_k + 16) >> 5 (arithmetic shift: the floor);  then one
 *   tap -- k = 1 for phi <= 32, k = 2 for phi > 32 -- is replaced by 16384 minus the other three, so every row sums to 16384.
 *   Wt[0] = (0, 16384, 0, 0), Wt[16] = (-1152, 14208, 3712, -384), Wt[32] = (-1024, 9216, 9216, -1024), Wt[63] = (-2, 136, 16374,
 *   -124); Wt[64 - phi] is Wt[phi] reversed; sum of |Wt[phi][k]| <= 20480; the smallest weight is -1213.
 *   lfg_sampling_weights writes the table, row-major 64 x 4; pure host code, no context.  NULL: LFG_ERR_INVALID.
 * The fetch of image img at position (px, py) in pixels, for the same P and C as the bilinear routes:
 *   u = px - 0.5f, fu = floorf(u), a = u - fu, and v, fv, b likewise (the bilinear fetch's own arithmetic);
 *   i = (int)fu, phix = (int)(a * 64.0f); j, phiy likewise.  (a rounds to 1.0f for a tiny negative u; the rule above at phi = 64
 *   gives (0, 0, 16384, 0), the texel at i + 1, and that row is used.)
 *   texel(r, k) = img(clamp(i - 1 + k, 0, W - 1), clamp(j - 1 + r, 0, H - 1)), r, k = 0 .. 3;  per channel c
 *       h_r = (sum over k of Wt[phix][k] * texel(r, k)_c + 64) >> 7          (arithmetic shift; |h_r| <= 40,800)
 *       s   = sum over r of Wt[phiy][r] * h_r                                 (|s| <= 835,584,000 < 2^31)
 *       p   = clamp((s + 4096) >> 13, 0, 65280)
 *   and the sample value is ((float)p / 255.0f) * 0.00390625f, the division correctly rounded.
 *   `inside` is the bilinear fetch's test, 0 <= px <= W and 0 <= py <= H; the inside rule, the blend mix(Pv, Cv, t), the clamp
 *   and the store follow unchanged, as do the gate, the projection, the key order and the hole rules before the fetch.
 * Hence: (1) where phix = phiy = 0, p = 256 texel and the value is the texel's UNORM value bit for bit, so whenever every fetched
 * position has integer u and v -- t = 0 and t = 1 with any vectors (t = 1 gives curr exactly), a uniform even vector at t = 0.5,
 * mvq = 4 mv under those conditions -- the output is the bilinear route's byte for byte;  (2) a constant frame stays constant at
 * every phase;  (3) a vertical step 40 | 200 fetched half a pixel off gives p / 256 = 30, 120, 210 across the edge: the overshoot
 * is the filter's and is kept, and at 0 | 255 the clamp of p engages on both sides.
 *
 * lfg_interpolate_compensated_sampled[_multi]: mv's format picks the route -- LFG_FORMAT_MV_S8X2 gives
 * lfg_interpolate_compensated[_multi]'s definition, LFG_FORMAT_MV_S16X2_Q2 lfg_interpolate_compensated_subpel[_multi]'s -- and
 * `sampling` the fetch.  With LFG_SAMPLING_BILINEAR the call is that existing call: same launches, same bytes.  With
 * LFG_SAMPLING_BICUBIC the route's clear and projection are followed by a sampling kernel with the fetch above; holes take the
 * 16 px walk whatever lfg_set_hole_reach says (no fill-plane variant is built).  Frames, checks, the lane's key image and the
 * stage timer are the existing call's; an unknown `sampling` is LFG_ERR_INVALID before anything is enqueued.
 * Not built, on purpose: masked, bidirectional, extrapolating and fill-plane variants; the shader interpolator; the gate's and
 * lfg_motion_subpel's prevq, which stay bilinear; anti-ringing of the fetch. */
typedef enum lfg_sampling { LFG_SAMPLING_BILINEAR = 0, LFG_SAMPLING_BICUBIC = 1 } lfg_sampling;
int  lfg_sampling_weights(int16_t weights[256]);
int  lfg_interpolate_compensated_sampled(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                         lfg_frame *out, float factor, int match_sad, int sampling);
int  lfg_interpolate_compensated_sampled_multi(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                                               lfg_frame *const *outs, const float *factors, uint32_t count, int match_sad,
                                               int sampling);
/* The fetch of lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else):
 *   LFG_SAMPLING_BILINEAR (default): every path enqueues and allocates what it did;
 *   LFG_SAMPLING_BICUBIC: exactly where those calls would run lfg_interpolate_compensated[_multi] with the 16 px walk, or, under
 *       lfg_set_subpixel_vectors, lfg_interpolate_compensated_subpel[_multi], the _sampled call with LFG_SAMPLING_BICUBIC runs in
 *       its place.
 * Under the shader interpolator, LFG_GENERATION_EXTRAPOLATE, lfg_set_static_protection, lfg_set_bidirectional or any
 * lfg_set_hole_reach the setting is stored and has no effect; lfg_sampling_effective then returns LFG_SAMPLING_BILINEAR -- it
 * returns what the next lfg_interpolate_frames call would fetch with (NULL: LFG_SAMPLING_BILINEAR) -- so a host can see that the
 * setting lapsed.  Any other value: LFG_ERR_INVALID and no change.  Measured cost and quality: DESIGN.md section 4.23. */
int  lfg_set_sampling(lfg_context *ctx, int sampling);
int  lfg_sampling_effective(const lfg_context *ctx);

/* Pair statistics: how well a vector field explains a pair of frames.  No reference counterpart.  A pair whose two frames do
 * not show the same scene (a cut, a cold start, a channel change) has no vectors that mean anything, and hardly any pixel
 * passes the compensated interpolator's match gate; moving content of every kind passes it almost everywhere (DESIGN.md
 * section 4.9: above 750 per thousand against below 30).  Integer arithmetic only; it does not depend on lfg_set_semantics.
 *   Inputs: prev, curr RGBA8 and mv LFG_FORMAT_MV_S8X2 (any byte values), all W x H; 0 <= match_sad <= 1020.
 *   With v = mv(q): sad(q) = sum over c of |curr(q)_c - prev(q + v)_c|, prev outside the image read as 0 -- the match gate of
 *   lfg_interpolate_compensated, word for word.
 *   pixels = W * H;  matched = the number of q with sad(q) <= match_sad;  sad_sum = the sum over q of sad(q).
 * All three are integers, so neither the order of evaluation nor any tiling changes a result.  The call WRITES the three
 * words of `device_stats` (24 bytes of device memory, 8-byte aligned): it does not accumulate into them.
 * Frames: 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4), 2-byte aligned mv.  Any violation, a NULL pointer or
 * a misaligned device_stats returns LFG_ERR_INVALID before anything is enqueued.  Enqueued on the selected lane (a clear of
 * the record, one launch of a fixed grid); keeps no device memory; timed under LFG_STAGE_MOTION. */
typedef struct lfg_pair_stats { uint64_t pixels, matched, sad_sum; } lfg_pair_stats;
int  lfg_pair_match(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                    int match_sad, void *device_stats /* 24 bytes of device memory, 8-byte aligned */);
/* The fallback of a cut: a source frame instead of a generated one.  No reference counterpart.  `device_stats` is a record as
 * lfg_pair_match writes it, read ON THE DEVICE when the call's turn on the lane comes: the host never waits for the verdict.
 *   The pair is a cut when matched * 1000 < min_matched_permille * pixels, in 64 bits; so 0 never cuts.
 *   A cut: every outs[i] becomes a copy of prev where factors[i] < 0.5f and of curr otherwise (a NaN factor: curr).  Only the
 *   width * 4 bytes of each row are written, never the row padding.  No cut: no byte of any output is written.
 * 0 <= min_matched_permille <= 1000, 1 <= count <= LFG_MAX_FACTORS; prev, curr and every output RGBA8 of one size, 4-byte
 * aligned rows, the outputs overlapping neither an input nor each other; device_stats 8-byte aligned.  Any violation or a
 * NULL pointer returns LFG_ERR_INVALID before anything is enqueued.  One launch of a small fixed grid on the selected lane,
 * for all outputs; every wave of it reads the record and returns if the pair is no cut.  Keeps no device memory; timed
 * under LFG_STAGE_INTERPOLATE. */
int  lfg_cut_fallback(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const void *device_stats,
                      int min_matched_permille, lfg_frame *const *outs, const float *factors, uint32_t count);
/* Cut detection in lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else).  No reference counterpart.
 *   min_matched_permille = -1 (default): off; every path as before;
 *   0 .. 1000: the vectors as before (the selected estimator, then the refinement if it is on); lfg_pair_match on those
 *       vectors with the context's match_sad (lfg_set_interpolator; 48 unless changed) into a record the lane owns; a copy of
 *       that record into pinned host memory with an event behind it; the selected interpolator as before; lfg_cut_fallback
 *       with this threshold on its outputs.  The outputs must then satisfy lfg_cut_fallback's rules as well, which are
 *       checked before anything is enqueued.  lfg_set_fused_motion_interpolate does not apply.  The record, its pinned copy
 *       and the event are made by a lane's first such call and freed with the lane.
 * Any other value: LFG_ERR_INVALID and no change.
 * lfg_last_pair_stats: the record of the SELECTED lane's last such call, and in *out_cut whether that call was a cut under the
 * threshold it ran with (either pointer may be NULL).  It waits for that record's event only -- if the lane has been
 * synchronised since, it returns at once -- and returns LFG_ERR_INVALID if the lane has made no such call.
 * What this does NOT do: it does not make a cut cheap.  The estimator and the interpolator still run, and the full search on an
 * uncorrelated 4K pair still costs about 7.5 ms; skipping that work would take the host waiting for
 * the verdict, or a change to the existing kernels.  lfg_motion_pyramid costs the same on any content, so on that route a cut
 * costs nothing extra. */
int  lfg_set_cut_detection(lfg_context *ctx, int min_matched_permille);   /* -1 (default): off; 0 .. 1000 */
int  lfg_last_pair_stats(lfg_context *ctx, lfg_pair_stats *out_stats, int *out_cut);

/* Frame comparison: how far two frames that live on the device are from each other.  No reference counterpart.  Integer
 * arithmetic only; it depends on no setting of the context.
 *   Inputs: a, b RGBA8, both W x H; channel_mask in 1 .. 15, bit c standing for channel c (byte c of the texel).
 *   For pixel q and channel c: d_c(q) = |a(q)_c - b(q)_c|;  m(q) = the largest d_c(q) over the channels of channel_mask.
 *   pixels = W * H;  sse[c] = the sum over q of d_c(q)^2, for all four channels whatever the mask;
 *   hist[k] = the number of q with m(q) = k.
 * All 261 words are 64-bit integers, so neither the order of evaluation nor any tiling changes a result.
 *   accumulate = 0: the call WRITES the 261 words of `device_stats` (2,088 bytes of device memory, 8-byte aligned);
 *   accumulate = 1: the call ADDS to them, pixels included: several pairs go into one record with no host wait between them.
 * Frames: 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4); a and b may overlap or be the same frame (nothing is
 * written to them); a view made with lfg_frame_wrap into a larger frame is a region of interest.  A NULL pointer, a wrong
 * format, differing sizes, a misaligned frame or record, a mask outside 1 .. 15 or any other value of accumulate returns
 * LFG_ERR_INVALID before anything is enqueued.  Enqueued on the selected lane (a clear of the record unless accumulate is 1,
 * one launch of a fixed grid); keeps no device memory; outside the stage timers (a comparison is no stage of the path). */
typedef struct lfg_frame_diff_stats { uint64_t pixels; uint64_t sse[4]; uint64_t hist[256]; } lfg_frame_diff_stats;   /* 2,088 bytes */
int  lfg_frame_diff(lfg_context *ctx, const lfg_frame *a, const lfg_frame *b, uint32_t channel_mask,
                    int accumulate, void *device_stats /* 2,088 bytes of device memory, 8-byte aligned */);
/* A record in HOST memory (copied from the device by the caller) as the figures one quotes.  A pure host function: no
 * context, no GPU.  channel_mask should be the one the record was made with: hist depends on that mask, sse does not.
 *   differing = pixels - hist[0];  over_1 = differing - hist[1] (the pixels beyond +-1 LSB);
 *   max_abs = the largest k with hist[k] > 0, 0 if there is none;
 *   pP for P = 50, 99 = the smallest k with 100 * (hist[0] + .. + hist[k]) >= P * pixels, in 64 bits;
 *   mse = (the sum of sse[c] over the channels of channel_mask) / (popcount(channel_mask) * pixels), in double;
 *   psnr_db = 10 * log10(65025 / mse), HUGE_VAL where mse is 0.
 * Returns LFG_ERR_INVALID for a NULL pointer, a mask outside 1 .. 15, pixels = 0 or a histogram that does not sum to
 * pixels (the record's own consistency check: a record of several masks, or one that was never written). */
typedef struct lfg_frame_diff_summary { uint64_t pixels, differing, over_1; uint32_t max_abs, p50, p99; double mse, psnr_db; } lfg_frame_diff_summary;
int  lfg_frame_diff_summarize(const lfg_frame_diff_stats *host_stats, uint32_t channel_mask, lfg_frame_diff_summary *out);

/* Level matching: what keeps the stages' vectors through a fade, a flash or an exposure change, where a piece of content no
 * longer has the same byte values in prev and curr.  Three device calls and one switch; none has a reference counterpart.
 * Integer arithmetic only; every result is exact and depends on no setting of the context (the switch apart).
 *
 * The histogram of a frame that lives on the device.  No reference counterpart.
 *   Input: frame RGBA8, W x H.  pixels = W * H;  hist[c][k] = the number of pixels whose byte c equals k, for all four channels.
 *   accumulate = 0: the call WRITES the 1,025 words of `device_stats` (8,200 bytes of device memory, 8-byte aligned);
 *   accumulate = 1: the call ADDS to them, pixels included: several frames go into one record with no host wait between them.
 * Frames: as lfg_frame_diff's -- 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4); a view made with
 * lfg_frame_wrap into a larger frame is a region of interest; row padding is never read into a count.  A NULL pointer, a wrong
 * format, a misaligned frame or record or any other value of accumulate returns LFG_ERR_INVALID before anything is enqueued.
 * Enqueued on the selected lane (a clear of the record unless accumulate is 1, one launch of a fixed grid); keeps no device
 * memory; outside the stage timers. */
typedef struct lfg_frame_histogram_stats { uint64_t pixels; uint64_t hist[4][256]; } lfg_frame_histogram_stats;   /* 8,200 bytes */
int  lfg_frame_histogram(lfg_context *ctx, const lfg_frame *frame, int accumulate,
                         void *device_stats /* 8,200 bytes of device memory, 8-byte aligned */);
/* A pair of monotone level maps from two histogram records, built ON THE DEVICE: the host never waits for a histogram.  No
 * reference counterpart.  A is the record at `device_hist_from`, B the one at `device_hist_to` (both as lfg_frame_histogram
 * writes them; they may be the same record); cdfX[c][v] = the sum of histX[c][u] over u <= v.  For c = 0, 1, 2 (alpha has no map):
 *   forward[c][v] = the smallest w with cdfB[c][w] >= cdfA[c][v]: a level of A to B's level of equal rank;
 *   inverse[c][w] = the smallest v with cdfA[c][v] >= cdfB[c][w];
 *       (255 where no such level exists, which only records of unequal counts can ask for)
 *   shift_sum = the sum over c < 3 and v of histA[c][v] * |forward[c][v] - v|;   pixels = A's pixels;   reserved = 0;
 *   active = 1 when A's and B's pixels are equal and non-zero and 16 * shift_sum >= (uint64_t)min_shift16 * 3 * pixels, in
 *       64 bits; otherwise active = 0 and BOTH maps are written as the identity (shift_sum stays what the rule gave).
 * min_shift16 is the mean level shift that makes a pair worth levelling, in sixteenths of a level, 0 .. 4080: 0 levels every
 * pair of equal size; a larger value leaves pairs alone whose histograms merely differ because content entered or left.
 * `device_map` is 1,560 bytes of device memory, 8-byte aligned, overlapping neither record.  A NULL or misaligned pointer or a
 * min_shift16 outside 0 .. 4080 returns LFG_ERR_INVALID before anything is enqueued.  One launch of one workgroup on the
 * selected lane; keeps no device memory; outside the stage timers. */
typedef struct lfg_levels_map { uint64_t pixels, shift_sum; uint32_t active, reserved;
                                uint8_t forward[3][256], inverse[3][256]; } lfg_levels_map;                        /* 1,560 bytes */
int  lfg_levels_match(lfg_context *ctx, const void *device_hist_from, const void *device_hist_to,
                      int min_shift16, void *device_map /* 1,560 bytes of device memory, 8-byte aligned */);
/* A map through every pixel of a frame.  No reference counterpart.  `device_map` is a map as lfg_levels_match writes it, read on
 * the device when the call's turn on the lane comes.
 *   LFG_LEVELS_FORWARD: out_c = forward[c][in_c] for c < 3; alpha is copied; `factor` is ignored.
 *   LFG_LEVELS_AT: tq = (int)floorf(factor * 256.0f + 0.5f), factor finite in [0, 1];
 *       out_c = ((256 - tq) * inverse[c][in_c] + tq * in_c + 128) >> 8 for c < 3; alpha is copied.  So factor 1 leaves a frame
 *       as it is and factor 0 takes a frame at B's levels back to A's: a frame generated between a levelled prev and curr, which
 *       is at curr's levels, is taken to the levels of its own time.
 * An inactive map gives a byte copy in both modes.  in and out RGBA8 of one size, 4-byte aligned rows; `out` may be `in`
 * itself (the pass is point-wise) and may overlap it in no other way.  Only the width * 4 bytes of a row are written.  Any
 * violation, a NULL pointer, another mode or (under LFG_LEVELS_AT) a factor outside [0, 1] returns LFG_ERR_INVALID before
 * anything is enqueued.  One launch on the selected lane; keeps no device memory; outside the stage timers. */
typedef enum lfg_levels_mode { LFG_LEVELS_FORWARD = 0, LFG_LEVELS_AT = 1 } lfg_levels_mode;
int  lfg_levels_apply(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, const void *device_map, int mode, float factor);
/* Level matching in lfg_interpolate_frames and lfg_interpolate_frames_multi (nothing else).  No reference counterpart.
 *   min_shift16 = -1 (default): off; every path enqueues and allocates what it always did;
 *   0 .. 4080: a call, in this order,
 *     1. checks every argument that a later step can refuse -- lfg_cut_fallback's rules for the frames, and every factor a
 *        finite number in [0, 1], on the shader route too --: LFG_ERR_INVALID with nothing enqueued;
 *     2. enqueues lfg_frame_histogram of prev and of curr into two records the lane owns, lfg_levels_match(prev's, curr's,
 *        min_shift16) into a map the lane owns, and lfg_levels_apply(LFG_LEVELS_FORWARD) from prev into prev', an RGBA8
 *        temporary of the lane (W x H, pitch 4 W, made again when the size changes);
 *     3. runs exactly as with the switch off and prev' in prev's place: the selected estimator, halving, refinement, sub-pixel
 *        vectors, the static mask, the backward field, lfg_pair_match and the selected interpolator or extrapolator all see
 *        prev'.  lfg_set_fused_motion_interpolate does not apply: the stages run;
 *     4. under LFG_GENERATION_INTERPOLATE takes every outs[i] through lfg_levels_apply(LFG_LEVELS_AT, factors[i]) in place;
 *        under LFG_GENERATION_EXTRAPOLATE with the compensated interpolator nothing: those frames are fetched from curr alone;
 *     5. with lfg_set_cut_detection on runs lfg_cut_fallback last, with the CALLER's prev and curr: a cut still gives byte
 *        copies of the caller's frames;
 *     6. copies the map's first three words (pixels, shift_sum, active and reserved) into pinned host memory with an event
 *        behind the copy.
 * So an inactive pair gives the bytes of the same call with the switch off, factor 1 still gives curr, and the setting
 * composes with every other one by substitution.  Per lane it keeps 4 W H + 2 * 8,200 + 1,560 bytes and the pinned words,
 * made by the lane's first such call and freed with the lane.  Any other value: LFG_ERR_INVALID and no change.
 * lfg_last_level_match: those words of the SELECTED lane's last such call (any pointer may be NULL).  It waits for that
 * copy's event only and returns LFG_ERR_INVALID if the lane has made no such call.
 * Known limit: the maps are global.  A HUD that does not fade while the scene does is levelled with the scene, and under
 * lfg_set_static_protection such a pixel is no longer equal in prev' and curr. */
int  lfg_set_level_matching(lfg_context *ctx, int min_shift16);      /* -1 (default): off; 0 .. 4080 */
int  lfg_last_level_match(lfg_context *ctx, uint64_t *out_shift_sum, uint64_t *out_pixels, int *out_active);

/* Structural similarity: an exact-integer SSIM of two frames that live on the device, beside lfg_frame_diff's squared error.
 * No reference counterpart.  Integer arithmetic only; it depends on no setting of the context.  The window layout and the
 * constants are those of the integer SSIM of x264 and of FFmpeg's ssim filter; those finish in float, this one in integers, so
 * the figures are comparable in kind and not digit for digit.
 *   Inputs: a, b RGBA8, both W x H with 8 <= W, H <= 262,144; channel_mask in 1 .. 15, bit c standing for channel c.
 *   Windows: the frame is cut into 4 x 4 blocks, bw = W >> 2 by bh = H >> 2 of them; the columns and rows past the last
 *   multiple of 4 are not looked at.  A window is 2 x 2 blocks (8 x 8 pixels) at every block position (wx, wy) with
 *   wx < bw - 1, wy < bh - 1: (bw - 1) * (bh - 1) windows at stride 4, overlapping.
 *   Per window and channel c, over its 64 pixels: s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b;
 *     vars = 64 ss - s1^2 - s2^2;  covar = 64 s12 - s1 s2;
 *     N = (2 s1 s2 + 416) (2 covar + 235963);  D = (s1^2 + s2^2 + 416) (vars + 235963), both signed 64-bit;
 *     Q_c = sign(N) floor(|N| 2^24 / D).
 *   (416 and 235963 are 0.01^2 255^2 64 and 0.03^2 255^2 64 63, rounded.  0 <= |N| <= D < 2^58, so Q_c is in [-2^24, 2^24];
 *   it is 2^24 exactly where the window is the same in both frames, and negative values occur: a checkerboard against its
 *   inverse.)
 *   windows = (bw - 1) (bh - 1);  sum[c] = the sum of Q_c over the windows, signed, for all four channels whatever the mask;
 *   with m = the smallest Q_c over the channels of channel_mask:  hist[max(m, 0) >> 18] counts the window -- bin 64 the
 *   windows identical in every masked channel, bin 0 every negative value as well;
 *   worst = the smallest key ((m + 2^24) << 32) | (wy << 16) | wx over the windows: the lowest value, then the topmost,
 *   then the leftmost window; all ones where there is none.
 * All 71 words are 64-bit integers, so neither the order of evaluation nor any tiling changes a result.
 *   accumulate = 0: the call WRITES the 71 words of `device_stats` (568 bytes of device memory, 8-byte aligned);
 *   accumulate = 1: the call ADDS to them: windows, sum and hist are added, worst becomes the minimum of both.
 * Frames: as lfg_frame_diff's -- 4-byte aligned RGBA8 rows (any pitch that is a multiple of 4); a and b may overlap or be the
 * same frame; a view made with lfg_frame_wrap into a larger frame is a region of interest.  A NULL pointer, a wrong format,
 * differing sizes, a misaligned frame or record, a mask outside 1 .. 15, any other value of accumulate, or a width or height
 * below 8 or above 262,144 returns LFG_ERR_INVALID before anything is enqueued.  Enqueued on the selected lane (a clear of the
 * record unless accumulate is 1, one launch of a fixed grid); keeps no device memory; outside the stage timers. */
typedef struct lfg_frame_ssim_stats { uint64_t windows; int64_t sum[4]; uint64_t hist[65]; uint64_t worst; } lfg_frame_ssim_stats;   /* 568 bytes */
int  lfg_frame_ssim(lfg_context *ctx, const lfg_frame *a, const lfg_frame *b, uint32_t channel_mask,
                    int accumulate, void *device_stats /* 568 bytes of device memory, 8-byte aligned */);
/* A record in HOST memory (copied from the device by the caller) as the figures one quotes.  A pure host function: no
 * context, no GPU.  channel_mask should be the one the record was made with: hist and worst depend on it, sum does not.
 *   ssim[c] = sum[c] / (windows * 2^24), in double, for all four channels;  all = the mean of ssim[c] over the channels of
 *   channel_mask;  db = -10 log10(1 - all), HUGE_VAL where all is 1;
 *   identical = hist[64];  below_half = hist[0] + .. + hist[31] (the windows with m < 0.5);
 *   worst_value = ((worst >> 32) - 2^24) / 2^24, in double;  worst_x = 4 wx, worst_y = 4 wy: the window's first pixel.
 * Returns LFG_ERR_INVALID for a NULL pointer, a mask outside 1 .. 15, windows = 0 or a histogram that does not sum to
 * windows. */
typedef struct lfg_frame_ssim_summary { uint64_t windows, identical, below_half; double ssim[4], all, db, worst_value; uint32_t worst_x, worst_y; } lfg_frame_ssim_summary;
int  lfg_frame_ssim_summarize(const lfg_frame_ssim_stats *host_stats, uint32_t channel_mask, lfg_frame_ssim_summary *out);

/* NV12 input and output: colour conversion between 4:2:0 YUV as decoders write it and encoders read it, and the RGBA8 frames of
 * every other call.  No reference counterpart (the reference captures and presents RGBA only, src/frame_manager.hpp:15).
 * Integer arithmetic only; it depends on no setting of the context.  NV12 is no lfg_format: the planes are described by an
 * lfg_nv12 of caller-owned device memory.
 *   Planes: y is W x H bytes, rows y_pitch >= W apart, any alignment; uv is W/2 x H/2 interleaved (Cb, Cr) byte pairs, rows
 *   uv_pitch >= W apart, uv_pitch even and uv 2-byte aligned.  W and H are even.
 *   Coefficients (lfg_yuv_coefficients, the numbers the kernels use): Kr, Kb = 0.299, 0.114 (LFG_YUV_BT601) or 0.2126, 0.0722
 *   (LFG_YUV_BT709), Kg = 1 - Kr - Kb; LFG_YUV_LIMITED: sy = 255/219, sc = 255/224, o = 16; LFG_YUV_FULL: sy = sc = 1, o = 0.
 *   Each is round(x * 2^14) of the real value x computed in double (none is a tie), but for three that make the rows sum exactly:
 *     to_rgb = {cY, cRV, cGU, cGV, cBU} = sy, 2 (1 - Kr) sc, 2 Kb (1 - Kb) / Kg sc, 2 Kr (1 - Kr) / Kg sc, 2 (1 - Kb) sc;
 *     to_yuv = {yR, yG, yB, uR, uG, uB, vR, vG, vB}: yR = Kr / sy, yB = Kb / sy, yG = round(2^14 / sy) - yR - yB;
 *       uR = -Kr / (2 (1 - Kb)) / sc, uB = 0.5 / sc, uG = -uR - uB;  vR = 0.5 / sc, vB = -Kb / (2 (1 - Kr)) / sc, vG = -vR - vB.
 *   Chroma at luma pixel (x, y), scaled by 8, with i = x >> 1, j = y >> 1 and C the Cb or the Cr plane, indices clamped to it:
 *     LFG_CHROMA_REPLICATE: c8 = 8 C[j][i];
 *     LFG_CHROMA_LEFT (MPEG-2 siting: co-sited with the even columns, midway between the rows):
 *       h(r) = 2 C[r][i] for even x, C[r][i] + C[r][i + 1] for odd x;
 *       c8 = 3 h(j) + h(j - 1) for even y, 3 h(j) + h(j + 1) for odd y.
 *   lfg_nv12_to_rgba: y' = Y - o, cb = cb8 - 1024, cr = cr8 - 1024;
 *     R = clamp((8 cY y' + cRV cr + 2^16) >> 17), G = clamp((8 cY y' - cGU cb - cGV cr + 2^16) >> 17),
 *     B = clamp((8 cY y' + cBU cb + 2^16) >> 17), A = 255; clamp to [0, 255], >> the arithmetic shift (floor).
 *   lfg_rgba_to_nv12: Y = clamp(o + ((yR R + yG G + yB B + 2^13) >> 14)).  The pair (i, j) from the channel sums S over the luma
 *     rows 2j and 2j + 1: LFG_CHROMA_REPLICATE the columns 2i, 2i + 1 with weight 1 (shift 16); LFG_CHROMA_LEFT the columns
 *     2i - 1, 2i, 2i + 1 with weights 1, 2, 1, the column index clamped to the image (shift 17);
 *     Cb = clamp(128 + ((uR S_R + uG S_G + uB S_B + 2^(shift - 1)) >> shift)), Cr likewise with the v row.  Alpha is ignored.
 *   Every intermediate fits 32 bits.  Hence a grey input gives Cb = Cr = 128 and, under the full range, R = G = B = Y.
 * Frames: W and H even and equal to the RGBA frame's (at most 8,388,480 x 524,280); the RGBA frame 4-byte aligned with a pitch
 * that is a multiple of 4; the output overlaps no input, and the two planes of an output do not overlap each other.  Any
 * violation, a NULL pointer or an unknown matrix, range or siting returns LFG_ERR_INVALID before anything is enqueued.  Each call
 * is one launch on the selected lane; it keeps no device memory and is outside the stage timers (a conversion is no stage of
 * the path).  Only the W (or W * 4) bytes of each output row are written, never the row padding.  Offset pointers into larger
 * planes are a region of interest (even offsets, so that the chroma pairs line up). */
typedef struct lfg_nv12 { void *y; void *uv; uint32_t width, height, y_pitch, uv_pitch; } lfg_nv12;  /* caller-owned device memory */
typedef enum { LFG_YUV_BT601 = 0, LFG_YUV_BT709 = 1 } lfg_yuv_matrix;
typedef enum { LFG_YUV_LIMITED = 0, LFG_YUV_FULL = 1 } lfg_yuv_range;
typedef enum { LFG_CHROMA_REPLICATE = 0, LFG_CHROMA_LEFT = 1 } lfg_chroma_siting;
int  lfg_nv12_to_rgba(lfg_context *ctx, const lfg_nv12 *in, lfg_frame *out, int matrix, int range, int siting);
int  lfg_rgba_to_nv12(lfg_context *ctx, const lfg_frame *in, const lfg_nv12 *out, int matrix, int range, int siting);
/* The coefficients above.  A pure host function: no context, no GPU.  LFG_ERR_INVALID for a NULL pointer or an unknown enum. */
int  lfg_yuv_coefficients(int matrix, int range, int32_t to_rgb[5], int32_t to_yuv[9]);

/* Contrast-limited sharpening of a presented frame.  No reference counterpart: the reference presents what scale.comp wrote
 * (src/scaler.cpp:479-536).  Integer arithmetic only; it depends on no setting of the context.
 *   Inputs: in, out RGBA8, both W x H with W, H >= 1; 0 <= strength <= 64.
 *   For pixel q = (x, y) and each of the four channels c (all four alike, as everywhere else in this ABI; a constant alpha is
 *   flat and so unchanged):
 *     C = in(x, y)_c;  N, S, W, E = in(x, y - 1)_c, in(x, y + 1)_c, in(x - 1, y)_c, in(x + 1, y)_c, the neighbour coordinates
 *     clamped to the frame -- the frame the caller described: a view made with lfg_frame_wrap is its own image, and nothing
 *     outside it is read;
 *     L = 4 C - N - S - W - E;  lo = min(C, N, S, W, E);  hi = max(C, N, S, W, E);
 *     out(x, y)_c = clamp(C + ((strength * L + 32) >> 6), lo, hi), >> the arithmetic shift (floor).
 *   Strength 64 is the classic kernel (0 -1 0 / -1 5 -1 / 0 -1 0) limited to the local range; strength 0 copies.
 *   |strength * L + 32| reaches 65,312: it fits 32 bits and does NOT fit a 16-bit half; L (+-1020) and the min / max do.
 *   Limited: a pixel never leaves the range of itself and its four neighbours.  So edges steepen, while hard steps, flat areas,
 *   linear ramps and every local extremum stay as they are (the upscale's ringing is not amplified, one-pixel strokes get no
 *   halo), and the minimum and the maximum of a frame do not move.
 * Where: at the presentation end only, on a copy.  A frame that a motion, mask, cut or interpolation call will read must stay
 * unsharpened: sharpening raises per-pixel differences, and the match gate, the static mask and the cut statistics are
 * thresholds on those differences.
 * Frames: in and out both RGBA8 and both W x H with W, H >= 1; rows 4-byte aligned, the pitch a multiple of 4; out overlaps no
 * byte of in (every output depends on its neighbours' inputs, so the call cannot run in place); frames of 2 GiB and more are
 * addressed with size_t offsets.  Any violation, a NULL pointer or NULL data, a wrong format or a strength outside 0 .. 64
 * returns LFG_ERR_INVALID before anything is enqueued, and latches a message.  Enqueued on the selected lane (one launch
 * through 16-byte accesses where base and pitch of both frames are multiples of 16, with a second one for the 1 .. 3 columns
 * past the last multiple of 4; one launch through 4-byte accesses otherwise); keeps no device memory; outside the stage
 * timers (like a conversion it is no stage of the path).  Only the W * 4 bytes of each output row are written, never the row
 * padding. */
int  lfg_sharpen(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int strength);

/* Debanding with dithered output of a presented frame, opt-in.  No reference counterpart.  Captured games and 8-bit video
 * carry gradients quantised to one level per band; upscaling widens the bands, lfg_sharpen leaves ramps alone and
 * lfg_denoise_temporal removes the noise that hid the steps.  This replaces a pixel by the average of four random taps
 * around it where that average is close to the pixel -- with two more bits than a byte has -- and dithers the result back to
 * 8 bits.  Integer arithmetic only; it depends on no setting of the context.
 *   Inputs: in, out RGBA8, both W x H with W, H >= 1;
 *     iterations I: 1 <= I <= 4;  threshold T: 0 <= T <= 64, in quarters of a level;  radius R: 1 <= R <= 32;
 *     grain G: 0 <= G <= 16, in quarters of a level;  seed: any value.
 *   The random source is h(k), all in uint32 arithmetic:
 *     k ^= k >> 16;  k *= 0x7feb352d;  k ^= k >> 15;  k *= 0x846ca68b;  k ^= k >> 16.
 *   For pixel (x, y) -- coordinates relative to the frame the caller described: a view made with lfg_frame_wrap is its own
 *   image, and nothing outside it is read -- r0 = h(x ^ h(y ^ h(seed))) and r_j = h(r0 + j).
 *   Channels 0, 1 and 2 are processed as follows; channel 3 is copied.
 *     1. v = 4 in(x, y)_c.
 *     2. For i = 1 .. I, with S = R i:
 *          ox = (((r_i & 0xFFFF) (2 S + 1)) >> 16) - S,  oy = (((r_i >> 16) (2 S + 1)) >> 16) - S;
 *          s = the sum of in_c at (x + ox, y + oy), (x - ox, y - oy), (x - oy, y + ox) and (x + oy, y - ox), every
 *          coordinate clamped to the frame;
 *          T_i = T / i (integer division);  if |s - v| <= T_i then v = s.
 *        The taps always come from `in`, never from a partial result: no pixel depends on another pixel's output, and no
 *        tiling or evaluation order changes a byte.
 *     3. Noise: b_c = byte c of r_5;  n_c = ((b_c (4 + 2 G)) >> 8) - G, which lies in [-G, G + 3] with mean 1.5.  At G = 0
 *        it is the unbiased stochastic rounding of a value with two fractional bits.
 *     4. out(x, y)_c = clamp((v + n_c) >> 2, 0, 255), >> the arithmetic shift (floor).
 *   The multiplies are 16 bits x at most 257 and 8 bits x at most 36: every intermediate but h's fits 24 bits.
 * Hence: a pixel whose v was never replaced comes out as it went in when G = 0 (v = 4 in, n in 0 .. 3).  T = 0 with G = 0
 * copies the frame (s = v = 4 in is the only sum accepted).  Flat areas and hard steps do not move: in a flat area every s
 * equals v, and between two flat areas more than T levels apart a sum with a tap on the other side differs from v by at least
 * that step and is refused.  After the iterations
 * |v - 4 in| <= T_1 + ... + T_I, so every output lies within ceil((sum T_i + G + 3) / 4) levels of its input.  Alpha never
 * changes.  The same seed repeats the same bytes; the caller changes it per presented frame so that the dither does not
 * stand still.
 * Where: at the presentation end only, after lfg_sharpen, on a copy.  A frame that a motion, mask, cut, level, denoise or
 * interpolation call will read must stay as it is: dither noise defeats the exact-match shortcut and exhausts every threshold
 * on per-pixel differences.
 * Frames: in and out both RGBA8 and both W x H with W, H >= 1; rows 4-byte aligned, the pitch a multiple of 4; out overlaps no
 * byte of in (every output depends on taps up to R I pixels away, so the call cannot run in place); frames of 2 GiB and more
 * are addressed with size_t offsets.  Any violation, a NULL pointer or NULL data, a wrong format or a parameter outside its
 * range returns LFG_ERR_INVALID before anything is enqueued, and latches a message.  Enqueued on the selected lane (one launch
 * through 16-byte accesses where base and pitch of both frames are multiples of 16, with a second one for the 1 .. 3 columns
 * past the last multiple of 4; one launch through 4-byte accesses otherwise); keeps no device memory; outside the stage
 * timers (like a conversion it is no stage of the path).  Only the W * 4 bytes of each output row are written, never the row
 * padding.
 *   lfg_deband_draw writes the draw of one pixel: offsets = ox_1, oy_1, ... ox_4, oy_4 exactly as above (zeros past I) and
 *   noise_bytes = b_0, b_1, b_2.  Pure host code, no context: it holds the rule to a model without a GPU.  A NULL pointer or
 *   iterations or radius outside their ranges: LFG_ERR_INVALID.
 * Not built, on purpose: a disc instead of the square draw; blue-noise or ordered dither; debanding fused into lfg_sharpen or
 * into the NV12 store; a switch of lfg_interpolate_frames. */
int  lfg_deband(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int iterations, int threshold, int radius, int grain,
                uint32_t seed);
int  lfg_deband_draw(uint32_t seed, uint32_t x, uint32_t y, int iterations, int radius, int32_t offsets[8], int32_t noise_bytes[3]);

/* Motion-compensated temporal denoising, opt-in, in the caller's loop.  No reference counterpart.  Every frame-taking stage
 * thresholds per-pixel differences (the full search's exact-match shortcut, the match gate, the static mask, the cut
 * statistics), and sensor or encoder noise is what exhausts those thresholds; this averages each pixel of the current frame
 * with the content that the pair's vectors point at in one or two reference frames, where that content fits.  Integer
 * arithmetic only; it depends on no setting of the context, lfg_set_semantics included.
 *   Inputs: curr, out and refs[i] RGBA8, all W x H with W, H >= 1; mvs[i] LFG_FORMAT_MV_S8X2, W x H, on curr's grid as
 *   lfg_motion(refs[i], curr) writes it, so that refs[i](q + v_i(q)) ~ curr(q) -- the match gate's reading; any byte values;
 *   count = 1 or 2; 0 <= radius <= 2; 1 <= tolerance <= 1020; 0 <= strength <= 256; 0 <= limit <= 255.
 *   Cost of reference i at pixel q (the convention of lfg_motion_refine's cost): c_i = the sum over texels r of the
 *   (2 radius + 1)^2 window centred on q, and over the four channels, of |curr(r)_c - refs[i](r + v_i(q))_c|; texels r outside
 *   the image are skipped, refs[i] outside the image reads as 0.  n = the number of window texels inside the image,
 *   L = tolerance * n.
 *   Weight: w_i = (strength * max(0, L - c_i)) >> 6, and w_i = 0 if q + v_i(q) lies outside the image.  D = L + sum w_i;
 *   a_i = (256 * w_i) / D, the floor division of unsigned 32-bit values; a_0 = 256 - sum a_i.
 *   Mix, per channel c, all four alike:  m_c = (a_0 * curr(q)_c + sum a_i * refs[i](q + v_i(q))_c + 128) >> 8;
 *   out(q)_c = clamp(m_c, curr(q)_c - limit, curr(q)_c + limit).
 *   Bounds: c_i <= 25,500, w_i <= 102,000, D <= 229,500, 256 * w_i < 2^32, a_0 >= 1: every intermediate fits 32 bits.
 * Hence: strength = 0 or limit = 0 copies curr.  A reference whose window differs by `tolerance` or more per texel on average
 * contributes nothing, so a wrong vector, an occlusion or a cut leaves curr as it is.  Every output byte lies within the range
 * of the bytes mixed and within curr +- limit.  Identical references (a clean, correctly compensated stream) give out = curr.
 * At strength 64 a perfect reference gets half the weight, at 192 three quarters: the recursive use, where refs[0] is the
 * previous call's out and mvs[0] the field of lfg_motion(that out, curr), which the interpolator of the pair can use as well
 * (INTEGRATION.md).
 * Frames: rows 4-byte aligned, RGBA8 pitches multiples of 4; mv 2-byte aligned; out overlaps no byte of any input (a pixel
 * reads its neighbours, so the call cannot run in place); offsets are size_t, as in lfg_sharpen.  Any violation, a NULL
 * pointer (refs, mvs and their first `count` entries included) or NULL data, a wrong format or a parameter out of range returns
 * LFG_ERR_INVALID before anything is enqueued, and latches a message.  LFG_FORMAT_MV_S16X2_Q2 fields are refused: a
 * quarter-pixel variant is out of scope.  One launch on the selected lane; keeps no device memory; outside the stage timers.
 * Only the W * 4 bytes of each output row are written, never the row padding. */
int  lfg_denoise_temporal(lfg_context *ctx, const lfg_frame *curr, const lfg_frame *const *refs, const lfg_frame *const *mvs,
                          int count, lfg_frame *out, int radius, int tolerance, int strength, int limit);

/* Resampling with a choice of filter and anti-aliased downscaling.  No reference counterpart: lfg_scale is the reference's
 * scale.comp, six Lanczos-3 taps per axis at every ratio, which point-samples once the ratio is far below 1 (at 3:1 the
 * output centres fall on texel centres, where Lanczos-3 is an impulse).  lfg_scale stays as it is; this is a separate call.
 * Everything past the table is integer arithmetic; it depends on no setting of the context.
 *   Filters, with support S: LFG_FILTER_NEAREST (one tap); LFG_FILTER_BILINEAR (the triangle 1 - |x|, S = 1);
 *   LFG_FILTER_CATMULL_ROM (the cubic with B = 0, C = 1/2, S = 2); LFG_FILTER_MITCHELL (the cubic with B = C = 1/3, S = 2);
 *   LFG_FILTER_LANCZOS2 and LFG_FILTER_LANCZOS3 (a sin(pi x) sin(pi x / a) / (pi x)^2, 1 at 0, 0 for |x| >= a; S = a = 2, 3).
 *   The cubic: for |x| < 1, ((12 - 9B - 6C)|x|^3 + (-18 + 12B + 6C)|x|^2 + (6 - 2B)) / 6; for 1 <= |x| < 2,
 *   ((-B - 6C)|x|^3 + (6B + 30C)|x|^2 + (-12B - 48C)|x| + (8B + 24C)) / 6.
 *   Table of one axis, `in` -> `out` samples (lfg_resample_taps): N(p, k) = (2k + 1) out - (2p + 1) in and D = 2 max(in, out);
 *   the taps of output p are the integers k with |N| < S D -- integers decide which taps exist, no float does -- and the raw
 *   weight of a tap is f(N / D) in double.  So the filter is evaluated at the distance between texel centre and output centre
 *   divided by max(1, in / out): stretched where the axis shrinks (anti-aliasing), the plain kernel where it grows.
 *   LFG_FILTER_NEAREST is the single tap k = floor((2p + 1) in / (2 out)) with weight 16384.  Then, in this order:
 *     1. each raw weight is divided by the sum of the row's raw weights, summed in tap order;
 *     2. each tap is folded onto clamp(k, 0, in - 1), weights that land on one texel added in tap order (edge replication):
 *        first[p] is the smallest folded index and count[p] the span, so first >= 0 and first + count <= in;
 *     3. q = rint(w * 16384), ties to even;
 *     4. 16384 - sum q is added to the first tap of largest |q|: every row sums to exactly 16384.
 *   A row of more than LFG_RESAMPLE_MAX_TAPS taps before folding (Lanczos-3 from about 10.6 : 1 on), or one with
 *   sum |q| > 32768, is refused: LFG_ERR_UNSUPPORTED.
 *   Pixels, horizontal first, all four channels alike, >> the arithmetic shift (floor):
 *     h (y, p)_c = sum_j wx[p][j] in(y, fx[p] + j)_c          exact in 32 bits
 *     h'(y, p)_c = (h + 128) >> 8                             fits 16 bits because sum |w| <= 32768
 *     v (q, p)_c = sum_j wy[q][j] h'(fy[q] + j, p)_c          |v| <= 32640 * 32768 < 2^31
 *     out(q, p)_c = clamp((v + 2^19) >> 20, 0, 255)
 *   With in == out every filter but Mitchell, which is no interpolating kernel, returns the input bytes.
 * Frames: in and out both RGBA8, of any sizes >= 1; rows 4-byte aligned, the pitch a multiple of 4 and at least 4 * width; out
 * overlaps no byte of in; row offsets are size_t.  A view made with lfg_frame_wrap is its own image: nothing outside it is
 * read.  Any violation, a NULL pointer or NULL data, a wrong format or an unknown filter returns LFG_ERR_INVALID, a table
 * that is refused LFG_ERR_UNSUPPORTED -- both before anything is enqueued, with a message latched.  Enqueued on the selected
 * lane as ONE launch (both passes; the horizontal pass of a tile stays in LDS) and timed under LFG_STAGE_SCALE.  The first
 * call for a (filter, in, out) triple of an axis builds its table with lfg_resample_taps and uploads it; the context keeps a
 * bounded number of them.  lfg_scale_last_kernel is not touched.  Only the W * 4 bytes of each output row are written. */
typedef enum {
    LFG_FILTER_NEAREST = 0, LFG_FILTER_BILINEAR = 1, LFG_FILTER_CATMULL_ROM = 2, LFG_FILTER_MITCHELL = 3, LFG_FILTER_LANCZOS2 = 4,
    LFG_FILTER_LANCZOS3 = 5
} lfg_filter;
#define LFG_RESAMPLE_MAX_TAPS 64
int  lfg_resample(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter);
/* The table above -- the one builder: lfg_resample uploads what this returns.  A pure host function: no context, no GPU.
 * first and count hold out_size entries, weights out_size * LFG_RESAMPLE_MAX_TAPS: row p starts at p * LFG_RESAMPLE_MAX_TAPS
 * and its entries from count[p] on are 0.  LFG_ERR_INVALID for a NULL pointer, a size of 0, an in_size of 2^31 or more (first
 * is an int32_t) or an unknown filter;
 * LFG_ERR_UNSUPPORTED for a refused table (the arrays are then undefined). */
int  lfg_resample_taps(int filter, uint32_t in_size, uint32_t out_size, int32_t *first, uint32_t *count, int16_t *weights);

/* lfg_resample with the ringing of its upscaling passes limited (anti-ringing, as the scalers of video players have it).  No
 * reference counterpart.  Lanczos and the cubics with negative lobes overshoot at every hard edge; here the result of a 1-D
 * pass whose axis grows may not leave the range of the two source samples that bracket the output position, and `strength`
 * S in 0 .. 64 mixes the clamped result with the plain one in 64ths.  Everything said of lfg_resample holds: frames, checks,
 * tables, LFG_ERR_INVALID / LFG_ERR_UNSUPPORTED before anything is enqueued, ONE launch on the selected lane, timed under
 * LFG_STAGE_SCALE, integer arithmetic past the table, no branch on the content.  A strength outside 0 .. 64 is LFG_ERR_INVALID.
 *   Bracket of output sample p on an axis of `in` -> `out` samples (lfg_resample_brackets): with N = (2p + 1) in - out and
 *   D = 2 out, a(p) = clamp(floor(N / D), 0, in - 1) and b(p) = clamp(ceil(N / D), 0, in - 1), in integers -- the ceiling and
 *   not floor + 1: where the output centre is a texel's centre the bracket is that texel.  For every filter of support >= 1
 *   and out > in, first[p] <= a <= b < first[p] + count[p]: both are taps.
 *   Where: a pass is anti-ringed if S > 0, the filter is not LFG_FILTER_NEAREST and the pass's axis grows strictly (out > in).
 *   Any other pass keeps lfg_resample's formula, and where no pass qualifies the call IS lfg_resample: the same kernel, the
 *   same launch, the same bytes.
 *   Horizontal pass, with h the exact sum of lfg_resample and per channel c:
 *     L = 16384 min(in(y, a)_c, in(y, b)_c), U = 16384 max(the same);  d = clamp(h, L, U) - h;  g = h + floor(d S / 64);
 *     h' = (g + 128) >> 8          in place of (h + 128) >> 8
 *   Vertical pass, with v the sum over those h':
 *     L = 16384 min(h'(a, p)_c, h'(b, p)_c), U = 16384 max(the same);  d = clamp(v, L, U) - v, |d| < 2^31;
 *     u = v + floor(d S / 64)      (exact: (d >> 6) S + (((d & 63) S) >> 6));  out = clamp((u + 2^19) >> 20, 0, 255)
 *   So S = 64 makes each qualifying pass an exact clamp; with both axes growing every output byte then lies within the four
 *   texels in({a_y, b_y}, {a_x, b_x}) of its channel; bilinear, whose weights are a convex combination of the bracket, gives
 *   lfg_resample's bytes at every S; a constant frame stays constant.
 * The first call for an (in, out) pair of a growing axis builds its brackets with lfg_resample_brackets and uploads them; the
 * context keeps a bounded number of them, like the tables.  For presented frames: a perceptual control. */
int  lfg_resample_antiring(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter, int strength);
/* The brackets above -- the one builder: lfg_resample_antiring uploads what this returns.  A pure host function: no context,
 * no GPU.  lo and hi hold out_size entries each (a and b).  LFG_ERR_INVALID for a NULL pointer, a size of 0 or an in_size of
 * 2^31 or more. */
int  lfg_resample_brackets(uint32_t in_size, uint32_t out_size, int32_t *lo, int32_t *hi);

/* lfg_resample with its sums formed in linear or in sigmoidal light.  No reference counterpart.  The bytes of an RGBA8 frame
 * are sRGB-encoded, and lfg_resample weights them as if they were light: one-pixel stripes 0 | 255 shrunk 2 : 1 come out 128,
 * where half the light is the byte 188 ("the gamma error in picture scaling").  Here each colour byte is decoded to 14 bits of
 * light, the sums are formed there and the result is encoded again.  In linear light an upscaling filter's undershoot on the
 * dark side of an edge reaches black, so players upscale through a sigmoidal curve on top of linear light that compresses both
 * ends of the range; a downscale averages and belongs in linear light.  Everything said of lfg_resample holds: frames, checks,
 * tables, taps, edge folding, LFG_ERR_INVALID / LFG_ERR_UNSUPPORTED before anything is enqueued, ONE launch on the selected lane,
 * timed under LFG_STAGE_SCALE, integer arithmetic past the tables, no branch on the content.
 *   Tables (lfg_light_tables), in double: E(c) = c / 12.92 for c <= 0.04045, else ((c + 0.055) / 1.055)^2.4;
 *   S(L) = 0.75 - ln(1 / (L scale + offset) - 1) / 6.5 with offset = 1 / (1 + e^(6.5 * 0.75)) and
 *   scale = 1 / (1 + e^(6.5 (0.75 - 1))) - offset (centre 0.75 and slope 6.5, as mpv and libplacebo have them; S(0) = 0, S(1) = 1).
 *     forward[b]       = floor(16383 f(b / 255) + 0.5),  f = E for LFG_LIGHT_LINEAR and S o E for LFG_LIGHT_SIGMOID;
 *     threshold[k - 1] = (forward[k - 1] + forward[k] + 1) >> 1  for k = 1 .. 255;
 *     to_byte(L)       = the number of thresholds <= L: monotone, and to_byte(forward[b]) = b.
 *   forward increases strictly (by at least 5 and 48), and no value comes nearer a rounding tie than 3.6e-4: every libm agrees.
 *   Pixels, horizontal first, per colour channel c (R, G, B), >> the arithmetic shift (floor):
 *     h (y, p)_c = sum_j wx[p][j] forward[in(y, fx[p] + j)_c]   exact in 32 bits, |h| < 2^29
 *     h'(y, p)_c = (h + 8192) >> 14                             in [-8192, 24575]
 *     v (q, p)_c = sum_j wy[q][j] h'(fy[q] + j, p)_c            |v| <= 32768 * 24575 < 2^31 - 8192
 *     out(q, p)_c = to_byte(clamp((v + 8192) >> 14, 0, 16383))
 *   Alpha is not light: its byte is lfg_resample's, by lfg_resample's formula.
 *   Where it is something else: light == LFG_LIGHT_GAMMA, or filter == LFG_FILTER_NEAREST (the tables round-trip), IS
 *   lfg_resample: the same kernel, the same launch, the same bytes.  LFG_LIGHT_SIGMOID with an axis that shrinks (out < in) is
 *   LFG_ERR_UNSUPPORTED and launches nothing.  Any other value of `light` is LFG_ERR_INVALID.
 *   So a constant frame stays constant, with in == out an interpolating filter (every one but Mitchell) returns the input
 *   bytes, and the alpha plane equals lfg_resample's byte for byte.
 * The first call in a mode builds its tables with lfg_light_tables and uploads them (1 KiB); the context keeps both modes'
 * until it is destroyed.  For presented frames: a picture control. */
typedef enum { LFG_LIGHT_GAMMA = 0, LFG_LIGHT_LINEAR = 1, LFG_LIGHT_SIGMOID = 2 } lfg_light;
int  lfg_resample_light(lfg_context *ctx, const lfg_frame *in, lfg_frame *out, int filter, int light);
/* The tables above -- the one builder: lfg_resample_light uploads what this returns.  A pure host function: no context, no
 * GPU.  LFG_ERR_INVALID for a NULL pointer, for LFG_LIGHT_GAMMA, which has no tables, and for any other value of `light`. */
int  lfg_light_tables(int light, uint16_t forward[256], uint16_t threshold[255]);

/* Edge-adaptive upscaling.  No reference counterpart.  Every filter of lfg_resample is separable and cannot tell along an edge
 * from across it; this call analyses, per output pixel, the direction and the strength of the luma gradient over the 2 x 2
 * texels that bracket it, weighs 12 taps with a window rotated to that gradient -- narrow across the edge, wide along it -- and
 * holds the result to the bracket's range (the EASU pass of FSR 1, of which lfg_sharpen is the RCAS half).  It depends on no
 * setting of the context, is enqueued on the selected lane as ONE launch, is timed under LFG_STAGE_SCALE and leaves
 * lfg_scale_last_kernel alone.  All integers; >> is the arithmetic shift (floor) and / floor division of non-negatives.
 *   Frames: both RGBA8, sizes >= 1; `out` at least as large as `in` on each axis (equal sizes are allowed), a shrinking axis
 *   is LFG_ERR_UNSUPPORTED.  Pitch, alignment, overlap, NULL and format rules are lfg_resample's; a violation is
 *   LFG_ERR_INVALID.  Both errors return before anything is enqueued, with a message latched.  A view is its own image:
 *   nothing outside it is read.  Only W * 4 bytes of each output row are written.
 *   Positions, per axis `in` -> `out` (lfg_upscale_edge_positions): N = (2p + 1) in - out and D = 2 out;
 *     base a(p) = floor(N / D), in -1 .. in - 1;  frac phi(p) = floor(256 (N - a D) / D), in 0 .. 255.
 *   Every texel coordinate is clamped to the frame when it is read.
 *   Per-texel analysis, a property of the source texel, not of the output pixel: luma L = R + 2 G + B; with l, r, u, d the
 *   clamped neighbours' luma and c the texel's own,
 *     dX = r - l, mX = max(|r - c|, |c - l|);  dY = d - u, mY = max(|d - c|, |c - u|).
 *   Per output pixel (px, py): fx = phi_x(px), fy = phi_y(py), ax = a_x(px), ay = a_y(py).  The four bracket texels are
 *   T(i, j) = (ax + i, ay + j) for i, j in {0, 1}, their weights w = (i ? fx : 256 - fx) (j ? fy : 256 - fy), and the weighted
 *   sums over the four DX = sum w dX, DY = sum w dY, AX = sum w |dX|, MX = sum w mX, and AY, MY likewise.
 *   1. Direction.  gx = DX >> 10, gy = DY >> 10; k is the smallest index in 0 .. 15 that maximises |gx COS[k] + gy SIN[k]|,
 *        COS = 256, 251, 237, 213, 181, 142, 98, 50, 0, -50, -98, -142, -181, -213, -237, -251
 *        SIN = 0, 50, 98, 142, 181, 213, 237, 251, 256, 251, 237, 213, 181, 142, 98, 50
 *   2. Edge strength.  level(A, M) = 0 if M = 0, else how many k' in {1, 2, 3, 4} have 4 A >= k' M;
 *      q = level(AX, MX)^2 + level(AY, MY)^2, in 0 .. 32.  A clean step or ramp has level 4, a one-pixel line level 0.
 *   3. Flat.  If max(|DX|, |DY|) < 4 * 65536, then k = 0 and q = 0.
 *   4. Shape (k, q) -> (A, B, C, lob, clp) (lfg_upscale_edge_shapes, the one builder): c = COS[k], s = SIN[k],
 *      m = max(|c|, |s|), stretch = (65536 + m / 2) / m, len = q^2, sx = 256 + (((stretch - 256) len) >> 10),
 *      sy = 256 - (len >> 3), lob = 2048 - ((1188 len) >> 10), clp = 2^24 / lob,
 *        A = (sx^2 c^2 + sy^2 s^2) >> 22,  B = ((sx^2 - sy^2) c s) >> 22 (signed: a floor),  C = (sx^2 s^2 + sy^2 c^2) >> 22.
 *      All five fit an int16_t: A, C <= 2047 and clp <= 19,508.
 *   5. Taps: the 4 x 4 texels (ax - 1 .. ax + 2, ay - 1 .. ay + 2) without the four corners, 12 in all.  For tap (i, j):
 *        ox = 256 i - fx, oy = 256 j - fy
 *        d2 = clamp((A ((ox ox) >> 4) + 2 B ((ox oy) >> 4) + C ((oy oy) >> 4)) >> 10, 0, clp)
 *        t1 = ((1638 d2) >> 12) - 4096;  b = ((25 ((t1 t1) >> 12)) >> 4) - 2304
 *        t2 = ((lob d2) >> 12) - 4096;   wt = (b ((t2 t2) >> 12)) >> 12
 *      -- EASU's window (25/16 (2/5 x^2 - 1)^2 - 9/16) (lob x^2 - 1)^2 in Q12.
 *   6. Result.  W = sum wt; for channel c, S_c = sum wt texel_c, all four channels alike;
 *        out_c = clamp((2 S_c + W) / (2 W), lo_c, hi_c)
 *      with lo_c and hi_c the minimum and the maximum of the four bracket texels in that channel.  W lies in 3,364 .. 8,356 for
 *      every shape and every (fx, fy), so the division is defined, and it is exact however the kernel forms it; a numerator
 *      below 0 ends at lo_c.  Every intermediate fits 32 bits.
 * Consequences: a constant frame stays constant; every output byte lies within its 2 x 2 bracket, so nothing overshoots;
 * in == out is allowed but is not the identity.
 * The first call for an (in, out) pair of an axis builds its positions and uploads them; the context keeps a bounded number
 * of them, like the tap tables, and one copy of the shape table.  For presented frames. */
int  lfg_upscale_edge(lfg_context *ctx, const lfg_frame *in, lfg_frame *out);
/* The positions above -- the one builder: lfg_upscale_edge uploads what this returns.  A pure host function: no context, no
 * GPU.  base and frac hold out_size entries each.  Any sizes are taken (for out_size < in_size base still is the floor, but
 * steps by more than 1).  LFG_ERR_INVALID for a NULL pointer, a size of 0 or a size of 2^31 or more. */
int  lfg_upscale_edge_positions(uint32_t in_size, uint32_t out_size, int32_t *base, uint8_t *frac);
/* The shape table above: shapes[(k * 33 + q) * 5 + 0 .. 4] = A, B, C, lob, clp.  A pure host function.  LFG_ERR_INVALID for
 * NULL. */
int  lfg_upscale_edge_shapes(int16_t shapes[16 * 33 * 5]);

/* The reference's own data flow keeps prev / curr at INPUT resolution (src/scaler.cpp:443,451): there the generated
 * frame is interpolated at input resolution and then upscaled like a captured one.  This does both in one call --
 * identical, byte for byte, to lfg_interpolate into a temporary followed by lfg_scale of that temporary -- and where
 * `out` is exactly twice the size of the inputs optionally in ONE kernel (lfg_set_fused_interpolate_scale): each input
 * row of the 2x scale kernel is then interpolated on the fly (shaders/interpolate.comp:15-40 arithmetic, rounded to
 * bytes as the stage would store it), so the generated frame never exists at input resolution in memory (SURVEY.md
 * 8(f) rank 1).  prev, curr, mv: same size; out: any size. */
int  lfg_interpolate_scale(lfg_context *ctx, const lfg_frame *prev, const lfg_frame *curr, const lfg_frame *mv,
                           lfg_frame *out, float factor);
/* Which of the two lfg_interpolate_scale uses at exactly 2x.  Default 0: the two stages through a context-owned frame
 * -- measured FASTER on MI355X at 1080p -> 4K (interpolate 5 us + scale 13 us against 33 us for the fused kernel: the
 * 16 MB the intermediate frame moves cost less than re-interpolating the five warm-up rows of every strip inside a
 * kernel that is bound by instruction issue, not by memory).  1: the fused kernel.  Results
 * are identical.  Also set by LFG_FUSED_INTERPOLATE_SCALE=1 in the environment at context creation. */
int  lfg_set_fused_interpolate_scale(lfg_context *ctx, int enabled);

/* Write the motion vectors as the reference's rgba32f image: vec4(mv.x, mv.y, 0, 1) per pixel
 * (shaders/motion.comp:56) into `device_rgba32f` (width*height*16 bytes, device memory). */
int  lfg_mv_export_rgba32f(lfg_context *ctx, const lfg_frame *mv, void *device_rgba32f);

/* ---------------------------------------------------------------- multi-GPU: the one exchange of the path */

/* Frame pairs are independent, so a batch shards one pair per GPU with no communication -- except that the batch can
 * share its previous frame, which then travels from the rank that owns it to every other rank as ONE broadcast per
 * frame (RCCL ncclBroadcast of width*height*bpp bytes as ncclUint8, over xGMI).  The
 * reference has a single queue and no communication (src/vulkan_context.cpp:130-151): no counterpart.
 *
 * One process (or thread) per GPU, one context each.  Rank 0 makes the id and hands its bytes to the other ranks by
 * any means it likes (a file, a socket, MPI, a torch.distributed store); then EVERY rank calls lfg_comm_init with the
 * same id -- a collective call that returns once all ranks have arrived.  librccl.so is opened the first time one of
 * these calls is made; without it they return LFG_ERR_UNSUPPORTED. */
#define LFG_COMM_ID_BYTES 128
typedef struct lfg_comm_id { char bytes[LFG_COMM_ID_BYTES]; } lfg_comm_id;
int  lfg_comm_unique_id(lfg_comm_id *out_id);
int  lfg_comm_init(lfg_context *ctx, int nranks, int rank, const lfg_comm_id *id);
int  lfg_comm_rank(const lfg_context *ctx);       /* -1 without a communicator */
int  lfg_comm_ranks(const lfg_context *ctx);      /*  0 without a communicator */
/* Broadcast a tightly packed frame (every rank passes its own frame of the same size and format) from `root`,
 * asynchronously on the context's communication stream: it starts once everything enqueued so far on EVERY lane of
 * the context has finished (the kernels still reading the frame on a receiver, the kernels producing it on the root,
 * whichever lane they were given to) and runs next to whatever is enqueued afterwards.  Nothing enqueued later, on any
 * lane, may touch the frame before that lane has passed an lfg_comm_wait() (or waits, lfg_lane_wait, for a lane that has). */
int  lfg_broadcast_frame(lfg_context *ctx, lfg_frame *frame, int root);
/* The same, ordered behind what the SELECTED lane has been given so far and behind nothing else.  For a caller that has
 * already ordered the selected lane behind the frame's last readers (on a receiver) or producers (on the root), e.g. with
 * lfg_lane_wait for the lane that marked (lfg_lane_mark) after reading it -- which is what a step with frames in flight
 * does anyway (linux-fg_amd/sharding.py, bench.py: step k waits for step k - 1's upscales, the last readers of the slot
 * that step k + 1's frame lands in).  With three frames in flight the call above makes the broadcast for step k + 1 wait
 * for ALL of step k - 1 and step k + 1 for the broadcast: two frames in flight and a bubble (measured on one MI355X
 * with a 170 us stand-in for the broadcast, NOTES_r05.md section 7).  Misuse corrupts frames; when in doubt use the call above. */
int  lfg_broadcast_frame_lane(lfg_context *ctx, lfg_frame *frame, int root);
/* Make everything enqueued on the SELECTED lane from now on wait (on the device) for ALL broadcasts issued so far.
 * Contract: the communication stream is in order and one event, re-recorded behind each broadcast, stands for every
 * broadcast before it -- so with two broadcasts in flight this waits for both, never for the older one alone (a caller
 * that double-buffers, like linux-fg_amd/sharding.py, waits for slot k before it issues k + 1 and loses nothing).  Other
 * lanes are not gated: they call lfg_comm_wait themselves or order behind this lane with lfg_lane_mark / lfg_lane_wait. */
int  lfg_comm_wait(lfg_context *ctx);
/* The HOST waits until every broadcast issued so far has completed (the counterpart of lfg_lane_sync). */
int  lfg_comm_sync(lfg_context *ctx);
/* Compute units kept free for the communicator.  RCCL's device kernel (gfx950: 256 threads, 261 - 280 vector registers
 * per lane, 19.7 KB of LDS per channel) cannot share a CU with a workgroup of the persistent motion prefilter kernel
 * (two of them fill a CU's register files), and those stay for the whole launch: 0.3 ms under a pan, 0.7 - 7 ms on noise,
 * uncorrelated content or a scene cut.  So while a context has a communicator, every stream the LIBRARY owns (the
 * context's own, the lanes') carries a CU mask that leaves 8 CUs -- one in each XCD -- alone, the communication stream
 * is masked to exactly those 8 (a high-priority stream that may use any CU does NOT find them: tools/probe_cu_reserve.hip),
 * RCCL's kernel is limited to as many channels (ncclConfig_t::maxCTAs), and the persistent grid is sized for the other 248.
 * lfg_comm_init makes those streams again (it waits for them first); lfg_comm_destroy gives the CUs back.
 * LFG_COMM_CUS=0|8|16|24|32 in the environment at context creation changes the number (0: no reservation).
 * A stream the CALLER supplied (lfg_context_set_stream) is not touched: create it with
 * hipExtStreamCreateWithCUMask and the mask lfg_comm_cu_mask returns (`words` 32-bit words, at least CUs / 32;
 * bit i set = CU i may be used) or accept that a broadcast waits for a persistent launch to end.
 * (A masked stream has default flags: it synchronises with the NULL stream, which the library itself never uses.) */
int  lfg_comm_reserved_cus(const lfg_context *ctx);      /* 0 without a communicator */
int  lfg_comm_cu_mask(const lfg_context *ctx, uint32_t *out_words, int words);
/* Diagnostic: enqueue, ordered like a broadcast and on the same stream, `workgroups` (1 .. 64) workgroups of
 * the footprint of RCCL's device kernel that stay `microseconds` each (csrc/comm_probe.hip).  A communicator of ONE
 * rank launches nothing for a broadcast; this is how a single GPU shows whether a broadcast would find a CU while the
 * lanes hold the chip (tests/test_gpu_comm.py).  lfg_comm_wait / lfg_comm_sync treat it as a broadcast. */
int  lfg_comm_probe(lfg_context *ctx, int workgroups, int microseconds, int every_lane /* ordered like lfg_broadcast_frame (1) or lfg_broadcast_frame_lane (0) */);
/* Device time of the LAST probe from "everything it was ordered behind has finished" to its own end, in milliseconds
 * (waits for it): its `microseconds` plus however long its workgroups waited for a CU. */
int  lfg_comm_probe_ms(lfg_context *ctx, float *out_ms);
/* Collective teardown (also done by lfg_context_destroy).  Idempotent. */
int  lfg_comm_destroy(lfg_context *ctx);

/* ---------------------------------------------------------------- diagnostics */

/* The motion kernel uses a hand-written correctly rounded sqrt (csrc/lfg_motion_common.hpp: exact_sqrt).  This
 * compares it on the device with the compiler's IEEE sqrtf for every float whose bit pattern lies
 * in [lo_bits, hi_bits] and returns the number of mismatches (expected 0).  Test-suite use only. */
int  lfg_selftest_sqrt(lfg_context *ctx, uint32_t lo_bits, uint32_t hi_bits, uint64_t *out_mismatches);

/* The 2x scale kernel cuts the in_height + 1 row steps (2 .. in_height + 2; step r emits output rows 2r-5 and 2r-4)
 * into one contiguous band per XCD and each band into strips of three lengths (csrc/scale.hip: scale_2x_strip_of, the
 * same function the kernel evaluates).  This returns strip `index` of XCD `xcd`: its first step and its number of
 * steps (0 = nothing left of the band) and how many strips an XCD has.  Host arithmetic only, no GPU needed.
 * Test-suite use: every step must belong to exactly one strip. */
int  lfg_diag_scale_2x_strip(uint32_t in_height, uint32_t xcd, uint32_t index, uint32_t *out_strips_per_xcd,
                             int32_t *out_first_step, int32_t *out_steps);

/* ---------------------------------------------------------------- measurement */

/* When enabled, every stage launch is bracketed by HIP events on the context's stream; the
 * accumulated device time and launch count per stage are read with lfg_profile_get() (which
 * synchronises).  Disabled by default; lfg_profile_reset() clears the accumulators. */
int  lfg_profile_enable(lfg_context *ctx, int enabled);
int  lfg_profile_reset(lfg_context *ctx);
int  lfg_profile_get(lfg_context *ctx, int stage, double *out_total_ms, uint64_t *out_launches);

#ifdef __cplusplus
}
#endif
#endif /* LINUXFG_HIP_H */
