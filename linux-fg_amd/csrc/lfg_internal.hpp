// Internal declarations shared by the C-ABI implementation and the kernel launchers.
// Not part of the public boundary (that is include/linuxfg_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "linuxfg_hip.h"
#include "lfg_motion_verdict.hpp"
#include "lfg_resample.hpp"
#include "lfg_table_cache.hpp"
#include "lfg_upscale_edge.hpp"

namespace lfg {

// What lfg_table_cache.hpp allocates, frees and copies with: the table caches' and the lane buffers' device.
struct HipDevice {
    static int allocate(void **p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static int release(void *p) { return (int)hipFree(p); }
    static int copy(void *dst, const void *host, size_t bytes) { return (int)hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice); }
};

// Per-axis Lanczos tables for one (inSize -> outSize) resample, as shaders/scale.comp:24-41
// computes them per output coordinate: first tap index (floor(pixelPos) - 2, unclamped) and six
// weights, pre-normalised by the sum of the in-range weights (the shader divides by totalWeight,
// scale.comp:48; the filter is exactly separable) and zeroed for taps
// the shader skips (scale.comp:34-37).
struct AxisTable {
    int in_size = 0, out_size = 0;
    std::pair<int, int> key() const { return {in_size, out_size}; }
    bool pattern_2x = false;      // start[2k] == k-3 and start[2k+1] == k-2 for every k
    uint8_t *d_base = nullptr;    // ONE allocation: start | weight | class | palette, each at a multiple of 256 bytes (hipMalloc's own alignment)
    int *d_start = nullptr;       // [out_size]
    float *d_weight = nullptr;    // [out_size][6]
    // pattern_2x tables only.  At exact 2x the shader's per-column fp32 arithmetic yields a handful of DISTINCT weight
    // rows (the nominal phase row for ~97 % of the columns, a few rounding variants, the renormalised border rows:
    // 31 rows at 1920 -> 3840), so the 2x kernel fetches a one-byte class per output column and the row from a small
    // palette that stays in L1, instead of 96 bytes of table per lane: d_class[p] indexes d_palette[class][8]
    // (six weights + two pad floats, 32-byte rows).  palette_rows == 0: too many distinct rows, not built.
    uint8_t *d_class = nullptr;   // [out_size rounded up to 4]
    float *d_palette = nullptr;   // [palette_rows][8]
    int palette_rows = 0;
    // pattern_2x tables of the VERTICAL axis: strips per XCD of the 2x kernel (scale.hip: scale_2x_strip_of).
    int strips_per_xcd = 0;
};

// uv[p] = ((float)p + 0.5f) / (float)size for p = 0 .. size - 1 (shaders/interpolate.comp:30): the normalised coordinate of a
// pixel centre depends on its column (row) alone, so the interpolate kernels read it from a table built once per size on the
// host -- the same fp32 division, bit for bit -- instead of five IEEE divisions per thread (the kernel was VALU-bound on them).
//
// Round 4: where nothing displaces the sample (a zero motion vector -- under the literal semantics the only vector whose samples
// stay inside the image) texture() is asked for uv[p] itself, and fl(uv[p] * size - 0.5) is texel p with fraction 0
// for most p but not for all: in fp32 102 of 3840 columns and 85 of 2160 rows miss by an ulp and get real bilinear weights.
// `centre` marks the p that hit (the sample IS texel p: no coordinate arithmetic, no weights).  For the x axis the groups of four
// pixels a thread works on ("quads") have one bit each in `goodMask`, set where all four pixels are centres: a wave covers 64
// consecutive quads and learns with one scalar load which of its lanes need the two-texel blends of interpolate.hip.
struct UvTable {
    int size = 0;
    int key() const { return size; }
    uint8_t *d_base = nullptr;      // ONE allocation: uv | centre | goodMask
    float *d_uv = nullptr;          // [size rounded up to 4]
    uint8_t *d_centre = nullptr;    // [size rounded up to 64]: 1 where the undisplaced sample of p is exactly texel p
    uint64_t *d_goodMask = nullptr; // [blocks]: bit l of word b: quad 64 b + l lies inside the axis and is all centres
    int blocks = 0;                 // ceil(quads / 64)
    // uv[p] without the table and without an IEEE division: q = (p + 0.5) * rcp, then one correction step,
    // q + fma(-q, size, p + 0.5) * rcp -- three instructions.  rcpExact: the host has checked that this reproduces uv[p] bit for bit
    // for EVERY p of this axis (it does for all the benchmark's sizes); otherwise the kernels read the table.
    float rcp = 0.0f;
    bool rcpExact = false;
};

// What the interpolate kernels take besides the frames (interpolate.hip).
struct InterpTables {
    const float *uvx = nullptr, *uvy = nullptr;
    const uint8_t *centreX = nullptr, *centreY = nullptr;
    const uint64_t *goodMask = nullptr;        // of the x axis
    float rcpW = 0.0f, rcpH = 0.0f;            // UvTable::rcp of the two axes
    int rcpExact = 0;                          // both axes' three-instruction uv is exact (UvTable::rcpExact)
};

// lfg_interpolate_frames in the north-star order (the reference: motion dispatch, then interpolate
// dispatch on the same grid, src/frame_manager.cpp:342-366): the motion kernels (8 / 16 paths) write the GENERATED frame from the
// vector they have just decided, while it is in a register -- csrc/lfg_interp.hpp: interpolate_pixel, the very function the
// interpolate kernel is made of -- and the motion-vector frame becomes an optional output.  data == nullptr: off.
struct FusedOut {
    uint8_t *data = nullptr;      // RGBA8, the size of curr
    int pitch = 0;
    float t = 0.5f;               // interpolationFactor
    int intended = 0;             // lfg_set_semantics: the vector divided by the image size before it displaces uv
    int storeMv = 1;              // 0: the caller has no use for the vectors (lfg_interpolate_frames' temporary)
};

// Words of a call's control area (MotionWorkspaceLayout::ctrl), cleared by the hint kernel with the rest of the area.
enum MotionCtrlWord : int {
    kCtrlNextUnit = 0,        // next plan unit to draw
    kCtrlUnitsDone = 1,       // plan units finished (only a running plan unit can push onto the queue)
    kCtrlNextSlot = 2,        // next queue slot to draw
    kCtrlOpenCount = 4,       // segments left to the resolve kernel (the length of openList)
    kCtrlHardCount = 5,       // tiles in which the lean kernel left a segment (the length of hardTiles)
    kCtrlLeanSettled = 6,     // segments the lean kernel settled / left: counted in -DLFG_LEAN_STATS builds only
    kCtrlLeanLeft = 7,
};

struct MotionWorkspaceLayout { size_t colBand, rowBand /* [height], [width] words of the strip kernel (motion_strip.hip), inside the control area the hint kernel clears */; size_t verdict /* byte offset of the call's verdict word, order32[kCand + 2] of its own order table; orderFlags: of [kCand] */, orderFlags; size_t list, umin, count, tileFlags, segDone, segMap, queueCount, ctrl, order, plan, auxList, auxUmin, auxCount,
                               queue, dynList, dynUmin, dynCount, dynInit, openList, merge, mergeBytes, leanTiles, hardTiles, plan2, total; int queueCap, slots, rimSplit, listMain, listAux, listDyn, leanCount, leanLaunch /* with the partial tiles behind them */, rimSplit2, units, units2, units2Static /* the second plan's units without the lean kernel's tiles, which come last in its table */, tiles, lastLean /* the lane's last call went by the second plan */; };
// Work units of the motion prefilter (motion_plan.hip: prefilter_plan).  A unit is a 56 x 64 tile, or one of nChunks
// contiguous parts of a tile's candidate order, or one 16-row segment of a tile with its four waves on four parts of
// the order; parts have private lists in the aux arrays (merged by the resolve kernel).
struct PrefilterPlan {               // passed by value to the kernels
    int tilesX, units;
    const uint32_t *unitMap;         // per unit: tile | (first) chunk << 20 | nChunks << 24 | segment unit << 28 | segment << 29
    const uint32_t *unitAux;         // per unit: index of its tile's first 56 x 64 block in the aux arrays (whole tiles: 0xFFFFFFFF)
    const uint32_t *tileMap;         // per tile: 0xFFFFFFFF (whole) or first aux index | nChunks << 24
    uint32_t *auxList;               // records: csrc/lfg_motion_common.hpp, Rec
    float *auxUmin;
    uint32_t *auxCount;
    // Segments handed over at run time (a whole tile's segment that finds no match after the first batches): a queue
    // of unitMap-style entries and their private lists in 16-row blocks; see motion_prefilter_kernel.
    uint32_t *segMap;                // per (tile, segment): 0, or first block | parts << 24 | 1 << 31
    uint32_t *queueCount;            // [0] entries pushed this call (may exceed queueCap: the excess was not handed over), [1] tiles flagged
    uint32_t *queue;                 // [queueCap] unit entries (0: not pushed yet); slot h's lists are blocks 4h .. 4h+3
    int queueCap;
    uint32_t *dynList;
    float *dynUmin;
    uint32_t *dynCount;
    uint32_t *dynInit;               // per handed-over segment: the 16 x 56 thresholds of the wave that handed it over
    int dynParts;                    // parts of the candidate order a handed-over segment is searched in: 8 (two workgroups) one frame at a time, 4 with frames in flight
    uint32_t *openList, *openCount;  // the segments left to the resolve kernel (tile * 4 + segment), appended as units end
    // Pixels the strip kernel has decided before this launch (motion_strip.hip; nullptr: that kernel did not run): colBand[y] bit 0 /
    // bit 1 = the left / right kStripCols columns of row y, rowBand[x] = the top / bottom kStripRows rows of column x
    // (lfg_motion_tile.hpp: strip_decided).  Rim units and the resolve kernel leave them alone.
    const uint32_t *colBand, *rowBand;
    // Calls that went through the lean kernel first (motion_lean.hip): the table's last units -- that kernel's tiles -- are not drawn
    // from the table; instead the tiles in which it LEFT a segment come from the list it wrote (hardCount: nullptr = no such call).
    int unitsStatic;
    const uint32_t *hardTiles, *hardCount;
    FusedOut fused;                  // the generated frame, written where the vectors are decided (off: data == nullptr)
};
struct PrefilterPlanHost {
    int tilesX = 0, tiles = 0, units = 0, auxUnits = 0;
    std::vector<uint32_t> unitMap, unitAux, tileMap;
    std::vector<uint32_t> leanTiles;     // the whole tiles the lean kernel may take first (motion_lean.hip: lean_tile_ok)
    std::vector<uint32_t> leanPartial;   // ... and rim tiles of which it takes the segments that lie inside the image: tile | mask of segments << 24
};

// Scratch of lfg_motion_pyramid (motion_pyramid.hip): byte offsets of levels 1 .. levels of both frames (RGBA8, rows of w * 4
// bytes) and of their vector fields (MV_S8X2, rows of w * 2 bytes); w / h[0] is the frame's own size.
constexpr int kPyramidMaxLevels = 4;
struct PyramidLayout {
    int levels = 0;
    uint32_t w[kPyramidMaxLevels + 1] = {}, h[kPyramidMaxLevels + 1] = {};
    size_t prev[kPyramidMaxLevels + 1] = {}, curr[kPyramidMaxLevels + 1] = {}, mv[kPyramidMaxLevels + 1] = {};
    size_t total = 0;
};

// One axis' table of lfg_resample for one (filter, in, out): what lfg_resample_taps returned, on the device in ONE allocation
// (first | count | weights, the weight rows `axis.stride` apart), and the tile plan it gives as a vertical table.
struct ResampleTable {
    int filter = 0;
    uint32_t in_size = 0, out_size = 0;
    std::tuple<int, uint32_t, uint32_t> key() const { return {filter, in_size, out_size}; }
    uint8_t *d_base = nullptr;
    ResampleAxis axis{};
    ResamplePlan plan{};
};

// The brackets of one growing axis for lfg_resample_antiring, keyed by (in, out) alone: what lfg_resample_brackets returned, on
// the device in one allocation (lo | hi).
struct ResampleBracketTable {
    uint32_t in_size = 0, out_size = 0;
    std::pair<uint32_t, uint32_t> key() const { return {in_size, out_size}; }
    uint8_t *d_base = nullptr;
    ResampleBracket bracket{};
};

// The positions of one axis for lfg_upscale_edge, keyed by (in, out): what lfg_upscale_edge_positions returned, on the device in
// one allocation (base | frac).
struct EdgePositionTable {
    uint32_t in_size = 0, out_size = 0;
    std::pair<uint32_t, uint32_t> key() const { return {in_size, out_size}; }
    uint8_t *d_base = nullptr;
    EdgeAxis axis{};
};

struct ProfileSlot {
    hipEvent_t begin = nullptr, end = nullptr;
    int stage = 0;
};

// Scene-cut detection behind lfg_interpolate_frames[_multi] (lfg_set_cut_detection): the lane's record on the device, the
// pinned copy that each detecting call refreshes, and the event behind that copy.  Made by the lane's first such call.
struct CutDetectState {
    lfg_pair_stats *device = nullptr;          // what lfg_pair_match writes and lfg_cut_fallback reads
    lfg_pair_stats *pinned = nullptr;          // host copy (lfg_last_pair_stats)
    hipEvent_t event = nullptr;                // recorded behind the copy
    bool recorded = false;                     // the lane has made a detecting call
    int permille = -1;                         // the threshold that call ran with
};

// Level matching behind lfg_interpolate_frames[_multi] (lfg_set_level_matching): both frames' histogram records and the map on
// the device (one allocation: from | to | map), the pinned copy of the map's first three words that each such call refreshes,
// and the event behind that copy.  Made by the lane's first such call.
struct LevelMatchState {
    uint8_t *device = nullptr;                 // 2 x lfg_frame_histogram_stats, then the lfg_levels_map
    uint64_t *pinned = nullptr;                // pixels, shift_sum, (active, reserved) (lfg_last_level_match)
    hipEvent_t event = nullptr;                // recorded behind the copy
    bool recorded = false;                     // the lane has made a levelling call
};

}  // namespace lfg

// What a lane (lfg_lanes: one of several frames in flight on a GPU) owns apart from the context: its stream, the temporaries
// and the motion workspace of its calls, the event other lanes wait for, and the verdicts its motion calls are launched by.
struct lfg_lane_state {
    hipStream_t own_stream = nullptr, stream = nullptr;
    lfg_frame mv_tmp{};                        // temporary of lfg_interpolate_frames
    lfg_frame mv_refined{};                    // ... and its refined vectors (lfg_set_vector_refinement), made on demand
    lfg_frame mv_bwd{}, mv_bwd_refined{};      // ... and the same two measured from curr to prev (lfg_set_bidirectional), made on demand
    lfg_frame half_prev{}, half_curr{}, mv_half{};   // ... and both frames halved and their vectors (lfg_set_half_resolution_motion), made on demand
    lfg_frame mid_tmp{};                       // temporary of lfg_interpolate_scale where the fused kernel does not apply
    // prefiltered motion path: scratch for one frame size, grown on demand
    lfg::DeviceBuffer motion_ws;
    uint32_t motion_ws_w = 0, motion_ws_h = 0;
    lfg::MotionWorkspaceLayout motion_ws_layout{};
    int motion_units = 0;                      // work units of the prefilter for the current workspace size
    // lfg_motion_pyramid: both frames' pyramids and the vector fields of levels 1 .. L, grown on demand
    lfg::DeviceBuffer pyramid_ws;
    // lfg_interpolate_compensated: the key image K of one factor (W * H words), grown on demand
    lfg::DeviceBuffer mc_keys;
    // lfg_set_hole_reach: the fill plane of that key image (W * H words), grown on demand
    lfg::DeviceBuffer mc_fill;
    // lfg_set_static_protection: the pair's static mask (W * H bytes), grown on demand
    lfg::DeviceBuffer static_mask;
    // lfg_set_subpixel_vectors: the quarter-pixel field of the pair (W x H MV_S16X2_Q2), made on demand, and
    // lfg_interpolate_compensated_subpel: the key image of that route (W * H 64-bit words), grown on demand
    lfg_frame mvq_tmp{};
    lfg::DeviceBuffer mcq_keys;
    // every DeviceBuffer above, for lane_release's one loop: a new one is added here, next to its declaration
    std::array<lfg::DeviceBuffer *, 6> buffers() { return {&motion_ws, &pyramid_ws, &mc_keys, &mc_fill, &static_mask, &mcq_keys}; }
    hipEvent_t mark = nullptr;                 // lfg_lane_mark
    bool marked = false;
    lfg::MotionVerdictState verdict;           // the order kernel's verdict on the lane's last call (lfg_motion_verdict.hpp)
    lfg::CutDetectState cut;                   // lfg_set_cut_detection: the record of the lane's last detecting call
    lfg::LevelMatchState levels;               // lfg_set_level_matching: the records and the map of the lane's last levelling call
    lfg_frame levelled_prev{};                 // ... and prev at curr's levels, made on demand
};

struct lfg_context {
    int device = 0;
    int device_cus = 0;                        // its compute units
    std::vector<lfg_lane_state> lanes;         // never empty: lfg_context_create makes lane 0, lfg_lanes the others
    int lane = 0;                              // the selected one
    lfg_lane_state &cur() { return lanes[(size_t)lane]; }
    const lfg_lane_state &cur() const { return lanes[(size_t)lane]; }
    // the k-th lane from the selected one on (k < lanes.size()): loops over every lane visit the selected one first
    lfg_lane_state &from_selected(size_t k) { return lanes[((size_t)lane + k) % lanes.size()]; }
    // lfg_motion_prediction_stats: calls whose verdict came back, and the guesses it contradicted (all lanes together)
    uint64_t pred_verdicts = 0, pred_lean_wrong = 0, pred_grid_wrong = 0, pred_second_wrong = 0;
    std::string error;
    // the per-size tables (lfg_table_cache.hpp has the contract): scale, interpolate, lfg_resample, lfg_resample_antiring, lfg_upscale_edge
    lfg::TableCache<lfg::AxisTable, lfg::HipDevice> tables;
    lfg::TableCache<lfg::UvTable, lfg::HipDevice> uv_tables;
    lfg::TableCache<lfg::ResampleTable, lfg::HipDevice> resample_tables;
    lfg::TableCache<lfg::ResampleBracketTable, lfg::HipDevice> resample_brackets;
    lfg::TableCache<lfg::EdgePositionTable, lfg::HipDevice> edge_positions;
    lfg::EdgeShape *edge_shapes = nullptr;     // lfg_upscale_edge_shapes on the device, made by the first lfg_upscale_edge
    uint32_t *light_tables[2] = {nullptr, nullptr};   // lfg_light_tables of LFG_LIGHT_LINEAR / _SIGMOID on the device (1 KiB each), made by the mode's first lfg_resample_light
    int motion_slots = 0;                      // prefilter workgroups resident at once on this device (0 = not queried yet)
    int rim_split_env = 0;                     // LFG_MOTION_RIM_SPLIT at context creation (0: unset -- the plan follows the lane count)
    int motion_mode = 0;                       // 0: prefilter + exact fallback, 1: exact kernel only
    int semantics = 0;                         // 0: the shaders as written, 1: "intended" (lfg_set_semantics)
    int estimator = 0;                         // lfg_interpolate_frames[_multi]: LFG_ESTIMATOR_FULL_SEARCH / _PYRAMID (lfg_set_motion_estimator)
    int interpolator = 0;                      // lfg_interpolate_frames[_multi]: LFG_INTERPOLATOR_SHADER / _COMPENSATED (lfg_set_interpolator)
    int match_sad = 48;                        // ... and the compensated interpolator's match gate
    int refine_radius = -1;                    // lfg_interpolate_frames[_multi]: lfg_motion_refine's radius, -1 = off (lfg_set_vector_refinement)
    int cut_permille = -1;                     // lfg_interpolate_frames[_multi]: lfg_cut_fallback's threshold, -1 = off (lfg_set_cut_detection)
    int static_tolerance = -1;                 // lfg_interpolate_frames[_multi]: lfg_static_mask's tolerance, -1 = off (lfg_set_static_protection)
    int generation = 0;                        // lfg_interpolate_frames[_multi]: LFG_GENERATION_INTERPOLATE / _EXTRAPOLATE (lfg_set_generation)
    int bidir_tolerance = -1;                  // lfg_interpolate_frames[_multi]: the bidirectional route's tolerance, -1 = off (lfg_set_bidirectional)
    int hole_reach = -1;                       // the compensated, masked and bidirectional calls: the fill plane's reach, -1 = off: the walk (lfg_set_hole_reach)
    int half_res_radius = -1;                  // lfg_interpolate_frames[_multi]: lfg_motion_expand's radius, -1 = off (lfg_set_half_resolution_motion)
    int subpel_radius = -1;                    // lfg_interpolate_frames[_multi]: lfg_motion_subpel's radius, -1 = off (lfg_set_subpixel_vectors)
    int level_shift16 = -1;                    // lfg_interpolate_frames[_multi]: lfg_levels_match's threshold, -1 = off (lfg_set_level_matching)
    int sampling = 0;                          // lfg_interpolate_frames[_multi]: LFG_SAMPLING_BILINEAR / _BICUBIC where the plain or sub-pixel kind runs (lfg_set_sampling)
    uint32_t *motion_tables = nullptr;         // device: [semantics][rank2scan | order32 | entryOfScan], then baseScan
    bool fuse_interpolate_scale = false;       // lfg_interpolate_scale: one fused kernel instead of the two stages (measured slower)
    bool fuse_motion_interpolate = false;      // lfg_interpolate_frames: the motion kernels write the generated frame themselves
    bool motion_hints = true;                  // per-call visiting order from sample-block hints (LFG_MOTION_HINTS=0: off)
    bool motion_lean = true;                   // whole interior tiles go through the lean kernel first (LFG_MOTION_LEAN=0: off)
    lfg::MotionKnobs knobs;                    // measurement knobs, read once at creation
    // the one exchange of the path (lfg_comm.cpp): an RCCL communicator, its stream and two events
    void *comm = nullptr;                      // ncclComm_t
    int comm_ranks = 0, comm_rank = 0;
    hipStream_t comm_stream = nullptr;
    hipEvent_t comm_ready = nullptr, comm_done = nullptr;
    bool comm_pending = false;                 // some broadcast has been issued on this communicator (comm_done has been recorded)
    hipEvent_t probe_begin = nullptr, probe_end = nullptr;     // lfg_comm_probe: device timestamps, ready and done
    int scale_last_kernel = -1;                // 0 generic, 1 exact 2x, 2 fused interpolate -> 2x (lfg_scale_last_kernel)
    int motion_last_tier = 0;                  // the persistent kernel's variant of the last lfg_motion on any lane (lfg_motion_last_variant)
    int comm_cus = 0;                          // CUs the library's own streams leave to the communicator's kernels (0: none reserved)
    // profiling
    bool profile = false;
    std::vector<lfg::ProfileSlot> prof_pending;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_free;
    double prof_ms[LFG_STAGE_COUNT] = {0, 0, 0};
    uint64_t prof_n[LFG_STAGE_COUNT] = {0, 0, 0};
};

// A stream of the library's own (lfg_capi.cpp): non-blocking; with `ctx->comm_cus` CUs reserved for a communicator, a stream whose
// CU mask leaves those free.  lfg_restream: every stream the library owns is made again under the current reservation.
hipError_t lfg_own_stream_create(const lfg_context *ctx, hipStream_t *out);
int lfg_restream(lfg_context *ctx);

namespace lfg {

// A kernel of the footprint of RCCL's device kernel (comm_probe.hip): what lfg_comm_probe puts where a broadcast would run.
hipError_t launch_comm_probe(hipStream_t s, int workgroups, int microseconds);

// Kernel launchers (scale.hip, motion_*.hip, interpolate.hip).  All enqueue on `s` and return the
// launch status; arguments have been validated by the caller.
hipError_t launch_scale_generic(hipStream_t s, const lfg_frame &in, const lfg_frame &out,
                                const AxisTable &tx, const AxisTable &ty);
hipError_t launch_scale_2x(hipStream_t s, const lfg_frame &in, const lfg_frame &out,
                           const AxisTable &tx, const AxisTable &ty);
bool scale_2x_supported(const lfg_frame &in, const lfg_frame &out);
hipError_t launch_interpolate_scale_2x(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                       const lfg_frame &out, const AxisTable &tx, const AxisTable &ty, float factor, bool intended);
int scale_2x_strips_per_xcd(int inH);
void scale_2x_strip_host(int inH, int xcd, int index, int &first, int &steps);
hipError_t launch_motion_tiled_8_16(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr,
                                    const lfg_frame &mv, const uint32_t *tileFlags, const uint32_t *rank2scan,
                                    unsigned long long *merge = nullptr, uint32_t *flaggedTiles = nullptr, const FusedOut &fused = FusedOut(),
                                    bool expectNothing = false, uint32_t *verdictWord = nullptr, uint32_t *hostWord = nullptr);
// Candidate tables of the blockSize 8 / searchRadius 16 paths for one tie-break rule (motion_order.hip: motion_tables).
constexpr int kMotionTableWords = 1092;     // 33 * 33 candidates + the sentinel, padded to a multiple of 4
void motion_tables(bool intended, uint32_t *rank2scan, uint32_t *order32, uint32_t *entryOfScan, uint32_t *baseScan);
// Prefiltered motion path (motion_plan.hip, motion_prefilter.hip): MotionWorkspaceLayout = byte offsets of its scratch arrays.
size_t motion_workspace_bytes(uint32_t width, uint32_t height, int slots, int rimSplit, int rimSplit2, MotionWorkspaceLayout *layout);   // rimSplit2: the plan used beside the lean kernel (0: none)
PrefilterPlanHost prefilter_plan(uint32_t width, uint32_t height, int slots, int rimSplit);   // rimSplit: 4 or 8 parts of the order per rim segment
int prefilter_slots();      // workgroups of the prefilter kernel the current device holds at once
hipError_t launch_motion_prefiltered_8_16(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr,
                                          const lfg_frame &mv, uint8_t *workspace, const MotionWorkspaceLayout &layout, int units,
                                          const uint32_t *rank2scan, const uint32_t *order32,
                                          const uint32_t *entryOfScan, const uint32_t *baseScan, bool useHints, bool framesInFlight,
                                          const FusedOut &fused = FusedOut(), bool lean = false, uint32_t *leanFlagHost = nullptr,
                                          int groupsCap = 0 /* persistent workgroups at most (0: as many as the device holds) */,
                                          bool expectNoFallback = false /* the lane's previous call flagged no tile: a small fallback launch */,
                                          const MotionKnobs &knobs = MotionKnobs(), bool rankIsScan = true,
                                          int tier = 0 /* 1: the persistent kernel's variant for moderate sensor noise (motion_prefilter_kernel<false, 1>) */);
// This call's visiting order (motion_order.hip): hint kernel (which also clears the call's control area) + order kernel.
hipError_t launch_motion_order(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, uint32_t *hints, uint32_t *callOrder,
                               const uint32_t *entryOfScan, const uint32_t *baseScan, uint32_t *clearFrom, int clearWords, bool framesInFlight);
// The literal chain for what the prefilter left open (motion_resolve.hip); list / umin / count: the image-shaped arrays.
hipError_t launch_motion_resolve(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, const uint32_t *list,
                                 const float *umin, const uint32_t *count, const uint32_t *tileFlags, int tilesX, const PrefilterPlan &sp,
                                 const uint32_t *rank2scan, const uint32_t *segDone, int groups);
// The lean kernel for whole interior tiles (motion_lean.hip): runs between the order kernel and the generic prefilter, marks the
// segments it settles in segDone; the generic kernel skips those.
bool lean_tile_ok(int tile, int tilesX, int W, int H);
bool lean_segment_ok(int tile, int seg, int tilesX, int W, int H);
bool lean_frames_ok(const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv);
hipError_t launch_motion_lean(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                              const uint32_t *order32, const uint32_t *rank2scan, bool rankIsScan /* the shaders' own tie order: ranks are scan indices */,
                              const uint32_t *leanTiles, int nTiles, int tilesX, uint32_t *segDone,
                              uint32_t *hardTiles, uint32_t *hardCount, uint32_t *stats, bool whateverTheVerdict);
// The strips a pan exposes (motion_strip.hip): runs behind the order kernel, decides its pixels completely and lists them in
// colBand / rowBand (cleared with the call's control area); the persistent kernel's rim units and the resolve kernel skip them.
bool strip_frames_ok(const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv);
hipError_t launch_motion_strip(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, const uint32_t *order32,
                               const uint32_t *rank2scan, bool rankIsScan, uint32_t *colBand, uint32_t *rowBand,
                               uint32_t *tileFlags, uint32_t *flagged, int flagTilesX, int ldsPad);
hipError_t launch_motion_generic(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr,
                                 const lfg_frame &mv, int block_size, int radius, bool intended);
hipError_t launch_interpolate(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr,
                              const lfg_frame &mv, const lfg_frame &out, float factor, bool intended, const InterpTables &tb);
hipError_t launch_interpolate_multi(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                    const lfg_frame *const *outs, const float *factors, int count, bool intended,
                                    const InterpTables &tb);
// Coarse-to-fine motion (motion_pyramid.hip): pyramid_workspace_bytes lays out the scratch for frames of this size, and
// launch_motion_pyramid enqueues the pyramids, the level-L search and the refinements into it.
size_t pyramid_workspace_bytes(uint32_t width, uint32_t height, int levels, PyramidLayout *layout);
hipError_t launch_motion_pyramid(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                 int levels, int coarseRadius, int refineRadius, uint8_t *workspace, const PyramidLayout &layout);
// The fill plane of a key image (hole_fill.hip): the row pass and the column pass, which read `keys` and write `plane`; pitches
// in words, reach in [1, LFG_HOLE_REACH_MAX], band = rows per workgroup of the column pass (0: kFillBand, lfg_mc.hpp).
hipError_t launch_hole_fill_plane(hipStream_t s, const uint32_t *keys, size_t keysPitchWords, uint32_t *plane, size_t planePitchWords,
                                  int W, int H, int reach, bool passStatic, int band = 0);
// Motion-compensated interpolation (interpolate_mc.hip): clears `keys` (W * H words), projects, interpolates; one factor.
// The three interpolating launchers with `fill` (W * H words; lfg_set_hole_reach): the fill plane of `reach` after the
// projection, and the sampling kernel that reads it where K is a hole.  fill == nullptr: the launches of before.
hipError_t launch_interpolate_compensated(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                          const lfg_frame &out, float factor, int matchSad, uint32_t *keys, uint32_t *fill = nullptr,
                                          int reach = 0);
// The same with a static mask (interpolate_mc.hip), and the mask of a pair (static_mask.hip): one launch.
hipError_t launch_interpolate_compensated_masked(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                                 const lfg_mask &mask, const lfg_frame &out, float factor, int matchSad, uint32_t *keys,
                                                 uint32_t *fill = nullptr, int reach = 0);
hipError_t launch_static_mask(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, int tolerance, const lfg_mask &out);
// Motion-compensated extrapolation (extrapolate_mc.hip): clears `keys` (W * H words), projects past time 1, samples curr; one factor.
hipError_t launch_extrapolate_compensated(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                          const lfg_frame &out, float ahead, int matchSad, uint32_t *keys);
// Bidirectional compensated interpolation (interpolate_bidir.hip): clears `keys` (W * H words), projects both fields, samples; one
// factor.  And the forward-backward check of field `a` against field `b` on its own: one launch.
hipError_t launch_interpolate_compensated_bidirectional(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &fwd,
                                                        const lfg_frame &bwd, const lfg_frame &out, float factor, int matchSad,
                                                        int tolerance, uint32_t *keys, uint32_t *fill = nullptr, int reach = 0);
hipError_t launch_motion_consistency(hipStream_t s, const lfg_frame &a, const lfg_frame &b, int tolerance, const lfg_mask &out);
// Per-pixel vector refinement (motion_refine.hip): mv_out(q) = the best-fitting of mv_in's 17 candidates around q; one launch.
hipError_t launch_motion_refine(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvIn,
                                const lfg_frame &mvOut, int radius);
// Half-resolution motion (motion_expand.hip): the pyramid's level rule for one frame into a pitched output, and mv_out(q) = the
// best-fitting doubled vector of mv_low's 3 x 3 neighbours above q, then the best of its +-1 steps; one launch each.
hipError_t launch_frame_halve(hipStream_t s, const lfg_frame &in, const lfg_frame &out);
hipError_t launch_motion_expand(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvLow,
                                const lfg_frame &mvOut, int radius);
// Quarter-pixel vectors: mvq_out(q) = the best of the nine half-pixel steps around 4 mv_in(q), then of the nine quarter-pixel
// steps around that (motion_subpel.hip), one launch; and the compensated interpolation along such a field
// (interpolate_subpel.hip): clears `keys` (W * H 64-bit words), projects, samples; one factor.
hipError_t launch_motion_subpel(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvIn,
                                const lfg_frame &mvqOut, int radius);
hipError_t launch_interpolate_compensated_subpel(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvq,
                                                 const lfg_frame &out, float factor, int matchSad, unsigned long long *keys);
// The bicubic fetch (interpolate_bicubic.hip; lfg_interpolate_compensated_sampled): the two routes' clear and projection on their
// own (interpolate_mc.hip, interpolate_subpel.hip), and the launchers that follow them with the bicubic sampling kernel.
hipError_t launch_compensated_projection(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, float factor,
                                         int matchSad, uint32_t *keys);
hipError_t launch_compensated_projection_subpel(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mvq,
                                                float factor, int matchSad, unsigned long long *keys);
hipError_t launch_interpolate_compensated_bicubic(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv,
                                                  const lfg_frame &out, float factor, int matchSad, uint32_t *keys);
hipError_t launch_interpolate_compensated_subpel_bicubic(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr,
                                                         const lfg_frame &mvq, const lfg_frame &out, float factor, int matchSad,
                                                         unsigned long long *keys);
// Scene-cut detection (pair_stats.hip): launch_pair_match clears the 24-byte record `stats` and enqueues the fixed grid that
// fills it; launch_cut_fallback enqueues the kernel that reads it and, on a cut, copies prev or curr over every output.
hipError_t launch_pair_match(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const lfg_frame &mv, int matchSad,
                             int deviceCus, void *stats);
hipError_t launch_cut_fallback(hipStream_t s, const lfg_frame &prev, const lfg_frame &curr, const void *stats, int minMatchedPermille,
                               const lfg_frame *const *outs, const float *factors, int count, int deviceCus);
// Frame comparison (frame_diff.hip): clears the 2,088-byte record `stats` unless `accumulate`, then enqueues the fixed grid
// that adds the pair's sums and histogram to it; 16-byte loads where base and pitch of both frames allow, dword loads otherwise.
hipError_t launch_frame_diff(hipStream_t s, const lfg_frame &a, const lfg_frame &b, uint32_t channelMask, bool accumulate,
                             int deviceCus, void *stats);
// Level matching (levels.hip): launch_frame_histogram clears the 8,200-byte record `stats` unless `accumulate`, then enqueues the
// fixed grid that fills it; launch_levels_match one workgroup that writes the 1,560-byte map; launch_levels_apply the map through
// `in` into `out` (tq: LFG_LEVELS_AT's factor in 256ths, lfg_levels.hpp).
hipError_t launch_frame_histogram(hipStream_t s, const lfg_frame &frame, bool accumulate, int deviceCus, void *stats);
hipError_t launch_levels_match(hipStream_t s, const void *from, const void *to, int minShift16, void *map);
hipError_t launch_levels_apply(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const void *map, int mode, int tq);
// Structural similarity (frame_ssim.hip): clears the 568-byte record `stats` (zeros, `worst` all ones) unless `accumulate`, then
// enqueues the fixed grid that adds the pair's windows to it; 16-byte loads where base and pitch of both frames allow, dword
// loads otherwise.  The frames are at least 8 x 8.
hipError_t launch_frame_ssim(hipStream_t s, const lfg_frame &a, const lfg_frame &b, uint32_t channelMask, bool accumulate,
                             int deviceCus, void *stats);
// Colour conversion (yuv_convert.hip): the coefficients of lfg_yuv_coefficients and the range's offset as the kernels take them;
// one launch each; yuv_grid_ok says whether a frame of this size fits the launch's grid.
struct YuvCoefficients { int32_t to_rgb[5]; int32_t to_yuv[9]; int32_t offset; };
bool yuv_grid_ok(uint32_t width, uint32_t height);
hipError_t launch_nv12_to_rgba(hipStream_t s, const lfg_nv12 &in, const lfg_frame &out, const YuvCoefficients &k, int siting);
hipError_t launch_rgba_to_nv12(hipStream_t s, const lfg_frame &in, const lfg_nv12 &out, const YuvCoefficients &k, int siting);
// Contrast-limited sharpening (sharpen.hip): the 16-byte kernel where base and pitch of both frames allow, with the dword
// kernel behind it for the 1 .. 3 columns past the last multiple of 4; the dword kernel alone otherwise.
hipError_t launch_sharpen(hipStream_t s, const lfg_frame &in, const lfg_frame &out, int strength);
// Debanding with dithered output (deband.hip): the same two routes and the same remainder launch as launch_sharpen.
hipError_t launch_deband(hipStream_t s, const lfg_frame &in, const lfg_frame &out, int iterations, int threshold, int radius, int grain,
                         uint32_t seed);
// Temporal denoising (denoise.hip): out = curr mixed with refs[i] displaced by mvs[i], i < count (1 or 2); one launch.
hipError_t launch_denoise_temporal(hipStream_t s, const lfg_frame &curr, const lfg_frame *const *refs, const lfg_frame *const *mvs,
                                   int count, const lfg_frame &out, int radius, int tolerance, int strength, int limit);
// Resampling (resample.hip): one launch, both passes; `plan` is the vertical table's.
hipError_t launch_resample(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const ResampleAxis &x, const ResampleAxis &y,
                           const ResamplePlan &plan);
// ... with anti-ringing (resample_antiring.hip): the same launch shape; sx / sy is the strength of the horizontal / vertical pass,
// 0 where that pass is not anti-ringed (its bracket is then not read), and not both are 0.
hipError_t launch_resample_antiring(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const ResampleAxis &x, const ResampleAxis &y,
                                    const ResamplePlan &plan, const ResampleBracket &bx, const ResampleBracket &by, int sx, int sy);
// ... in linear or sigmoidal light (resample_light.hip): the same launch shape with 1 KiB more LDS; `tables` is the mode's
// forward[256] | threshold[255], 0xFFFF on the device, as uint16_t.
hipError_t launch_resample_light(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const ResampleAxis &x, const ResampleAxis &y,
                                 const ResamplePlan &plan, const uint32_t *tables);
// Edge-adaptive upscaling (upscale_edge.hip): one launch; `shapes` is the table on the device, 528 rows.
hipError_t launch_upscale_edge(hipStream_t s, const lfg_frame &in, const lfg_frame &out, const EdgeAxis &x, const EdgeAxis &y,
                               const EdgeShape *shapes);
hipError_t launch_mv_export(hipStream_t s, const lfg_frame &mv, float *rgba32f);
hipError_t launch_sqrt_selftest(hipStream_t s, uint32_t lo_bits, uint32_t hi_bits, unsigned long long *d_mismatch);

}  // namespace lfg
