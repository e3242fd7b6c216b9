// ref_driver.inc -- binds caller memory to one generated shader and dispatches it.  TEST INFRASTRUCTURE ONLY.
//
// Included at the end of each file oracle/ref_recipe.py generates, after the shader's edited text in namespace LFG_REF_NS, with
// exactly one of LFG_REF_SCALE / LFG_REF_MOTION / LFG_REF_INTERPOLATE defined.  This file is this project's own code and holds
// no shader text: it knows the shaders by the names of their bindings and push constants only.
//
// What it takes from the reference's Vulkan host code is READ there, not executed: one sampler for every binding (LINEAR,
// CLAMP_TO_EDGE, normalised coordinates), push constants in the declared order, and ceil(size / 16) workgroups of 16 x 16
// per axis, so that the last row and column of groups reach past the image and the shaders' own bounds returns run.
//
// A region [x0, x1) x [y0, y1) in output pixels runs as every whole workgroup that overlaps it (all of them for the whole
// image); stores outside the region are dropped (glsl::image2D's window), so pixels outside it keep what the caller put there.
// Bindings and push constants are namespace-scope variables of the generated file, so one call runs at a time (a mutex);
// within a call the workgroups are handed to `nthreads` threads, each with its own gl_GlobalInvocationID.
#include <atomic>
#include <mutex>
#include <thread>
#include <vector>

namespace {

constexpr int kGroup = 16;                               // layout(local_size_x = 16, local_size_y = 16)
std::mutex g_call;

// `mask`, where given, receives per invocation inside the image whether a fetch through a report_fraction sampler had a
// non-zero fractional weight (1) or not (0); it is W x H bytes and only the invocations that ran are written.
int dispatch(int W, int H, int x0, int y0, int x1, int y1, int nthreads, uint8_t *mask) {
    if (x0 < 0 || y0 < 0 || x1 > W || y1 > H || x0 > x1 || y0 > y1) return -1;
    if (x0 == x1 || y0 == y1) return 0;
    const int gx0 = x0 / kGroup, gy0 = y0 / kGroup;
    const int gx1 = (x1 + kGroup - 1) / kGroup, gy1 = (y1 + kGroup - 1) / kGroup;     // the whole image: ceil(size / 16)
    const int across = gx1 - gx0, groups = across * (gy1 - gy0);
    std::atomic<int> next{0};
    auto work = [&]() {
        for (int g = next.fetch_add(1); g < groups; g = next.fetch_add(1)) {
            const int gx = gx0 + g % across, gy = gy0 + g / across;
            for (int ly = 0; ly < kGroup; ly++) {
                for (int lx = 0; lx < kGroup; lx++) {
                    const int x = gx * kGroup + lx, y = gy * kGroup + ly;        // past W or H in the last groups: the shader returns
                    glsl::gl_GlobalInvocationID = glsl::uvec3((unsigned)x, (unsigned)y, 0u);
                    glsl::texture_fraction_seen = false;
                    LFG_REF_NS::shader_main();
                    if (mask && x >= x0 && y >= y0 && x < x1 && y < y1)
                        mask[(size_t)y * (size_t)W + (size_t)x] = glsl::texture_fraction_seen ? 1 : 0;
                }
            }
        }
    };
    if (nthreads > groups) nthreads = groups;
    if (nthreads > 64) nthreads = 64;
    std::vector<std::thread> pool;
    for (int i = 1; i < nthreads; i++) pool.emplace_back(work);
    work();
    for (auto &t : pool) t.join();
    return 0;
}

glsl::sampler2D frame_sampler(const uint8_t *p, int W, int H) {
    glsl::sampler2D s;
    s.data = p; s.width = W; s.height = H; s.format = glsl::Format::RGBA8;
    return s;
}

glsl::image2D windowed(void *p, int W, int H, glsl::Format f, int x0, int y0, int x1, int y1) {
    glsl::image2D i;
    i.data = p; i.width = W; i.height = H; i.format = f;
    i.x0 = x0; i.y0 = y0; i.x1 = x1; i.y1 = y1;
    return i;
}

}  // namespace

#if defined(LFG_REF_SCALE)
// scale: sampler `inputImage`, rgba8 image `outputImage`, push constants { ivec2 inputSize; ivec2 outputSize; }
extern "C" __attribute__((visibility("default")))
int ref_scale(const uint8_t *in, int inW, int inH, uint8_t *out, int outW, int outH, int x0, int y0, int x1, int y1, int nthreads) {
    if (!in || !out || inW <= 0 || inH <= 0 || outW <= 0 || outH <= 0) return -1;
    std::lock_guard<std::mutex> lock(g_call);
    LFG_REF_NS::inputImage = frame_sampler(in, inW, inH);
    LFG_REF_NS::outputImage = windowed(out, outW, outH, glsl::Format::RGBA8, x0, y0, x1, y1);
    LFG_REF_NS::pc.inputSize = glsl::ivec2(inW, inH);
    LFG_REF_NS::pc.outputSize = glsl::ivec2(outW, outH);
    return dispatch(outW, outH, x0, y0, x1, y1, nthreads, nullptr);
}

#elif defined(LFG_REF_MOTION)
// motion: samplers `previousFrame`, `currentFrame`, rgba32f image `motionVectors`, push constants { ivec2 imageSize;
// int blockSize; float searchRadius; }.  mv_xy takes the stored texel's .xy, mv_zw (may be null) its .zw.
extern "C" __attribute__((visibility("default")))
int ref_motion(const uint8_t *prev, const uint8_t *curr, int W, int H, int blockSize, float searchRadius,
               float *mv_xy, float *mv_zw, int x0, int y0, int x1, int y1, int nthreads) {
    if (!prev || !curr || !mv_xy || W <= 0 || H <= 0 || blockSize < 0 || !(searchRadius >= 0.0f)) return -1;
    std::lock_guard<std::mutex> lock(g_call);
    LFG_REF_NS::previousFrame = frame_sampler(prev, W, H);
    LFG_REF_NS::currentFrame = frame_sampler(curr, W, H);
    LFG_REF_NS::motionVectors = windowed(mv_xy, W, H, glsl::Format::RG32F_OF_RGBA32F, x0, y0, x1, y1);
    LFG_REF_NS::motionVectors.zw = mv_zw;
    LFG_REF_NS::pc.imageSize = glsl::ivec2(W, H);
    LFG_REF_NS::pc.blockSize = blockSize;
    LFG_REF_NS::pc.searchRadius = searchRadius;
    return dispatch(W, H, x0, y0, x1, y1, nthreads, nullptr);
}

#elif defined(LFG_REF_INTERPOLATE)
// interpolate: samplers `previousFrame`, `currentFrame`, `motionVectors` (over the rgba32f image, its .xy from mv_xy), rgba8
// image `outputFrame`, push constants { float interpolationFactor; ivec2 imageSize; }.  `mask` (may be null): see dispatch().
extern "C" __attribute__((visibility("default")))
int ref_interpolate(const uint8_t *prev, const uint8_t *curr, const float *mv_xy, int W, int H, float factor,
                    uint8_t *out, uint8_t *mask, int x0, int y0, int x1, int y1, int nthreads) {
    if (!prev || !curr || !mv_xy || !out || W <= 0 || H <= 0) return -1;
    std::lock_guard<std::mutex> lock(g_call);
    LFG_REF_NS::previousFrame = frame_sampler(prev, W, H);
    LFG_REF_NS::currentFrame = frame_sampler(curr, W, H);
    glsl::sampler2D vectors;
    vectors.data = mv_xy; vectors.width = W; vectors.height = H;
    vectors.format = glsl::Format::RG32F_OF_RGBA32F; vectors.report_fraction = true;
    LFG_REF_NS::motionVectors = vectors;
    LFG_REF_NS::outputFrame = windowed(out, W, H, glsl::Format::RGBA8, x0, y0, x1, y1);
    LFG_REF_NS::pc.interpolationFactor = factor;
    LFG_REF_NS::pc.imageSize = glsl::ivec2(W, H);
    return dispatch(W, H, x0, y0, x1, y1, nthreads, mask);
}

#else
#error "define one of LFG_REF_SCALE, LFG_REF_MOTION, LFG_REF_INTERPOLATE"
#endif
