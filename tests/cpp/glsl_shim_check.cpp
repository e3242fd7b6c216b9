// Test helper (CPU only): known answers for oracle/glsl_shim.hpp, the GLSL built-ins the executed reference shaders run on --
// the ones where a slip would go unnoticed because the oracle could share it.  Built with g++ alone, plainly and with
// -fsanitize=address,undefined.  With -DLFG_HAVE_REF_SHADERS the generated oracle/_ref/*.cpp are linked in and each shader
// also runs once on a tiny image whose buffers are exactly as large as the image, so a fetch or a store past either is the
// sanitizer's.  Prints "ok <checks>" and exits 0, or prints each failed check and exits 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "glsl_shim.hpp"

#ifdef LFG_HAVE_REF_SHADERS
extern "C" {
int ref_scale(const uint8_t *in, int inW, int inH, uint8_t *out, int outW, int outH, int x0, int y0, int x1, int y1, int nthreads);
int ref_motion(const uint8_t *prev, const uint8_t *curr, int W, int H, int blockSize, float searchRadius,
               float *mv_xy, float *mv_zw, int x0, int y0, int x1, int y1, int nthreads);
int ref_interpolate(const uint8_t *prev, const uint8_t *curr, const float *mv_xy, int W, int H, float factor,
                    uint8_t *out, uint8_t *mask, int x0, int y0, int x1, int y1, int nthreads);
}
#endif

namespace {

using namespace glsl;

int checks = 0, failures = 0;

#define CHECK(cond) do { ++checks; if (!(cond)) { ++failures; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } } while (0)

std::vector<uint8_t> ramp_frame(int w, int h, int seed) {
    std::vector<uint8_t> f((size_t)w * h * 4);
    uint32_t s = 2463534242u + (uint32_t)seed;
    for (auto &b : f) { s ^= s << 13; s ^= s >> 17; s ^= s << 5; b = (uint8_t)(s >> 11); }
    return f;
}

sampler2D sampler_of(const std::vector<uint8_t> &f, int w, int h) {
    sampler2D s;
    s.data = f.data(); s.width = w; s.height = h;
    return s;
}

bool same(vec4 a, vec4 b) { return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w; }

uint8_t stored(float v) {                                // one texel through imageStore, first channel
    uint8_t px[4] = {7, 7, 7, 7};
    image2D img;
    img.data = px; img.width = 1; img.height = 1; img.x1 = 1; img.y1 = 1;
    imageStore(img, ivec2(0, 0), vec4(v, 0.0f, 0.0f, 0.0f));
    return px[0];
}

void conversions() {
    const ivec2 t(vec2(-2.5f, 2.5f));                    // towards zero, not floor and not nearest
    CHECK(t.x == -2 && t.y == 2);
    const ivec2 u(vec2(-0.75f, 16.0f));
    CHECK(u.x == 0 && u.y == 16);
    const vec2 f(ivec2(-3, 7));
    CHECK(f.x == -3.0f && f.y == 7.0f);
    const uvec3 id(5u, 9u, 0u);
    const ivec2 p(id.xy);
    CHECK(p.x == 5 && p.y == 9);
    const vec4 v(vec2(1.5f, -2.0f), 0.0f, 1.0f);
    CHECK(v.xy.x == 1.5f && v.xy.y == -2.0f && v.z == 0.0f && v.w == 1.0f);
    CHECK(vec4(0.25f).w == 0.25f && vec2(3.0f).y == 3.0f && ivec2(4).x == 4 && ivec2(4).y == 4);
}

void common_functions() {
    CHECK(fract(-0.25f) == 0.75f);                       // x - floor(x), not the C fmod
    CHECK(fract(-2.0f) == 0.0f && fract(1.5f) == 0.5f);
    const vec2 fr = fract(vec2(-1.75f, 3.25f));
    CHECK(fr.x == 0.25f && fr.y == 0.25f);
    const vec2 fl = floor(vec2(-0.5f, 2.75f));
    CHECK(fl.x == -1.0f && fl.y == 2.0f);
    CHECK(sin(0.0f) == 0.0f);
    CHECK(sin(3.14159265359f) == (float)std::sin((double)3.14159265359f));         // (4): through double, ~ -8.7e-8, not 0
    CHECK(sin(3.14159265359f) != 0.0f);
    // (9): x*(1-a) + y*a, which is not x + a*(y-x): at a = 0.3 the two differ in the last bit for these values
    const float x = 0.7f, y = 0.1f, a = 0.3f;
    CHECK(mix(x, y, a) == x * (1.0f - a) + y * a);
    CHECK(mix(5.0f, 9.0f, 0.0f) == 5.0f && mix(5.0f, 9.0f, 1.0f) == 9.0f && mix(2.0f, 4.0f, 0.5f) == 3.0f);
    const vec4 m = mix(vec4(0.0f, 1.0f, 2.0f, 3.0f), vec4(4.0f, 5.0f, 6.0f, 7.0f), 0.25f);
    CHECK(same(m, vec4(1.0f, 2.0f, 3.0f, 4.0f)));
    // (7): ((dx^2 + dy^2) + dz^2) + dw^2.  With 2^24 first and three ones after it, every one is absorbed in that order;
    // pairwise or reversed summation would give sqrt(2^24 + 2) or more.
    const vec4 big(4096.0f, 1.0f, 1.0f, 1.0f), zero(0.0f);
    CHECK(distance(big, zero) == 4096.0f);
    const vec4 rev(1.0f, 1.0f, 1.0f, 4096.0f);
    CHECK(distance(rev, zero) == std::sqrt(16777216.0f + 3.0f) && distance(rev, zero) != 4096.0f);
    CHECK(distance(vec4(1.0f, 2.0f, 3.0f, 4.0f), vec4(1.0f, 2.0f, 0.0f, 0.0f)) == 5.0f);
}

void relational() {
    CHECK(any(lessThan(vec2(-1.0f, 2.0f), vec2(0.0f))) && !any(lessThan(vec2(0.0f, 0.0f), vec2(0.0f))));
    CHECK(any(greaterThan(vec2(0.5f, 1.5f), vec2(1.0f))) && !any(greaterThan(vec2(1.0f, 1.0f), vec2(1.0f))));
    CHECK(any(lessThan(ivec2(3, -1), ivec2(0))) && !any(lessThan(ivec2(0, 0), ivec2(0))));
    CHECK(any(greaterThanEqual(ivec2(3, 4), ivec2(8, 4))) && !any(greaterThanEqual(ivec2(7, 3), ivec2(8, 4))));
    CHECK(!any(greaterThanEqual(vec2(0.5f, 0.5f), vec2(1.0f))) && any(greaterThan(ivec2(2, 0), ivec2(1, 1))));
}

void fetches() {
    const int w = 8, h = 4;
    const std::vector<uint8_t> f = ramp_frame(w, h, 1);
    const sampler2D s = sampler_of(f, w, h);
    const vec4 t = texelFetch(s, ivec2(3, 2), 0);
    const uint8_t *p = &f[(2 * w + 3) * 4];
    CHECK(same(t, vec4(p[0] / 255.0f, p[1] / 255.0f, p[2] / 255.0f, p[3] / 255.0f)));    // (1)
    for (const ivec2 q : {ivec2(-1, 0), ivec2(0, -1), ivec2(w, 0), ivec2(0, h), ivec2(-5, 9)})
        CHECK(same(texelFetch(s, q, 0), vec4(0.0f)));                                      // (5)
    // (3) at exact centres of a power-of-two image: (x + 0.5) / 8 and its product with 8 are exact, so the weights are 1, 0
    for (int y = 0; y < h; y++)
        for (int x = 0; x < w; x++)
            CHECK(same(texture(s, vec2(((float)x + 0.5f) / (float)w, ((float)y + 0.5f) / (float)h)), texelFetch(s, ivec2(x, y), 0)));
    // CLAMP_TO_EDGE: at uv 0 and 1 both taps of that axis are the edge texel with weights 0.5 and 0.5, which add to 1 exactly;
    // the other axis at a centre.  In a corner all four taps are the corner texel at 0.25 each, summed in the documented order.
    const float cy = 1.5f / (float)h, cx = 2.5f / (float)w;
    CHECK(same(texture(s, vec2(0.0f, cy)), texelFetch(s, ivec2(0, 1), 0)));
    CHECK(same(texture(s, vec2(1.0f, cy)), texelFetch(s, ivec2(w - 1, 1), 0)));
    CHECK(same(texture(s, vec2(cx, 0.0f)), texelFetch(s, ivec2(2, 0), 0)));
    CHECK(same(texture(s, vec2(cx, 1.0f)), texelFetch(s, ivec2(2, h - 1), 0)));
    for (const ivec2 corner : {ivec2(0, 0), ivec2(1, 0), ivec2(0, 1), ivec2(1, 1)}) {
        const vec4 e = texelFetch(s, ivec2(corner.x * (w - 1), corner.y * (h - 1)), 0);
        const vec4 got = texture(s, vec2((float)corner.x, (float)corner.y));
        CHECK(got.x == ((0.25f * e.x + 0.25f * e.x) + 0.25f * e.x) + 0.25f * e.x);
        CHECK(got.w == ((0.25f * e.w + 0.25f * e.w) + 0.25f * e.w) + 0.25f * e.w);
        CHECK(std::fabs(got.y - e.y) <= 1.2e-7f && std::fabs(got.z - e.z) <= 1.2e-7f);
    }
    // half way between two centres: the plain mean, in the documented order
    const vec4 a = texelFetch(s, ivec2(2, 1), 0), b = texelFetch(s, ivec2(3, 1), 0);
    const vec4 mid = texture(s, vec2(3.0f / (float)w, 1.5f / (float)h));
    CHECK(mid.x == 0.5f * a.x + 0.5f * b.x && mid.w == 0.5f * a.w + 0.5f * b.w);
    // a vector image: .xy from memory, z = 0 and w = 1, and the fraction report
    const float mv[2 * 3 * 2] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12};
    sampler2D v;
    v.data = mv; v.width = 3; v.height = 2; v.format = Format::RG32F_OF_RGBA32F; v.report_fraction = true;
    CHECK(same(texelFetch(v, ivec2(1, 1), 0), vec4(9.0f, 10.0f, 0.0f, 1.0f)));
    texture_fraction_seen = false;
    const vec4 centre = texture(v, vec2(0.5f, 0.25f));                           // u = 1.0, v = 0.0 exactly
    CHECK(same(centre, vec4(3.0f, 4.0f, 0.0f, 1.0f)) && !texture_fraction_seen);
    const vec4 between = texture(v, vec2(0.5f, 0.5f));                           // v = 0.5: rows 0 and 1 in equal parts
    CHECK(texture_fraction_seen && between.x == 6.0f && between.y == 7.0f && between.z == 0.0f && between.w == 1.0f);
    texture_fraction_seen = false;
    texture(s, vec2(0.3f, 0.3f));                                                // a frame's sampler does not report
    CHECK(!texture_fraction_seen);
}

void stores() {
    CHECK(stored(0.0f) == 0 && stored(1.0f) == 255 && stored(0.5f) == 128);      // 127.5 is a tie: to even, 128
    // exact ties that fp32 reaches through the store's own product v * 255.0f (each premise is checked beside its answer)
    CHECK(stored(0.1f) == 26);                           // 25.5 exactly in fp32 (0.1f * 255.0f rounds to 25.5): even is 26
    CHECK(0.1f * 255.0f == 25.5f);
    CHECK(stored(0.3f) == 76);                           // 76.5 exactly (0.3f * 255.0f == 76.5f): even is 76
    CHECK(0.3f * 255.0f == 76.5f);
    CHECK(stored(-0.25f) == 0 && stored(1.75f) == 255 && stored(-0.0f) == 0);    // clamping
    CHECK(stored(std::numeric_limits<float>::quiet_NaN()) == 0);
    CHECK(stored(std::numeric_limits<float>::infinity()) == 255 && stored(-std::numeric_limits<float>::infinity()) == 0);
    // outside the image and outside the window nothing is written; rg32f stores .xy and, where asked, .zw
    uint8_t px[2 * 2 * 4] = {0};
    image2D img;
    img.data = px; img.width = 2; img.height = 2; img.x0 = 1; img.y0 = 0; img.x1 = 2; img.y1 = 2;
    imageStore(img, ivec2(2, 0), vec4(1.0f));
    imageStore(img, ivec2(0, -1), vec4(1.0f));
    imageStore(img, ivec2(0, 1), vec4(1.0f));            // inside the image, outside the window
    bool untouched = true;
    for (uint8_t b : px) untouched = untouched && b == 0;
    CHECK(untouched);
    imageStore(img, ivec2(1, 1), vec4(1.0f, 0.0f, 1.0f, 0.0f));
    CHECK(px[12] == 255 && px[13] == 0 && px[14] == 255 && px[15] == 0 && px[8] == 0);
    float xy[2 * 2] = {0}, zw[2 * 2] = {0};
    image2D vi;
    vi.data = xy; vi.zw = zw; vi.width = 2; vi.height = 1; vi.format = Format::RG32F_OF_RGBA32F; vi.x1 = 2; vi.y1 = 1;
    imageStore(vi, ivec2(1, 0), vec4(vec2(-16.0f, 2.5f), 0.0f, 1.0f));
    CHECK(xy[2] == -16.0f && xy[3] == 2.5f && zw[2] == 0.0f && zw[3] == 1.0f && xy[0] == 0.0f && zw[1] == 0.0f);
}

#ifdef LFG_HAVE_REF_SHADERS
void shaders() {
    // sizes that are no multiple of the 16 x 16 workgroup, so the shaders' bounds returns run; heap buffers of exactly the
    // image's size; two threads, so the thread-local invocation id is exercised
    const int iw = 7, ih = 5, ow = 19, oh = 18;
    const std::vector<uint8_t> in = ramp_frame(iw, ih, 2);
    std::vector<uint8_t> up((size_t)ow * oh * 4, 0);
    CHECK(ref_scale(in.data(), iw, ih, up.data(), ow, oh, 0, 0, ow, oh, 2) == 0);
    bool constant_alpha = true;
    std::vector<uint8_t> flat((size_t)iw * ih * 4, 200), flat_up((size_t)ow * oh * 4, 0);
    CHECK(ref_scale(flat.data(), iw, ih, flat_up.data(), ow, oh, 0, 0, ow, oh, 1) == 0);
    for (uint8_t b : flat_up) constant_alpha = constant_alpha && b == 200;       // a constant frame scales to itself
    CHECK(constant_alpha);
    std::vector<uint8_t> part((size_t)ow * oh * 4, 0);
    CHECK(ref_scale(in.data(), iw, ih, part.data(), ow, oh, 3, 2, 18, 17, 2) == 0);
    bool window = true;
    for (int y = 0; y < oh; y++)
        for (int x = 0; x < ow; x++)
            for (int c = 0; c < 4; c++) {
                const size_t at = ((size_t)y * ow + x) * 4 + c;
                const bool inside = x >= 3 && x < 18 && y >= 2 && y < 17;
                window = window && part[at] == (inside ? up[at] : 0);
            }
    CHECK(window);
    CHECK(ref_scale(in.data(), iw, ih, up.data(), ow, oh, 0, 0, ow + 1, oh, 1) == -1);

    const int w = 21, h = 17;
    const std::vector<uint8_t> prev = ramp_frame(w, h, 3);
    std::vector<uint8_t> curr((size_t)w * h * 4, 0);
    for (int y = 0; y < h; y++)                          // curr(q) = prev(q + (2, -1)), 0 outside
        for (int x = 0; x < w; x++)
            if (x + 2 < w && y - 1 >= 0)
                for (int c = 0; c < 4; c++) curr[((size_t)y * w + x) * 4 + c] = prev[((size_t)(y - 1) * w + x + 2) * 4 + c];
    std::vector<float> xy((size_t)w * h * 2, 99.0f), zw((size_t)w * h * 2, 99.0f);
    CHECK(ref_motion(prev.data(), curr.data(), w, h, 4, 3.0f, xy.data(), zw.data(), 0, 0, w, h, 2) == 0);
    const size_t mid = ((size_t)8 * w + 9) * 2;
    CHECK(xy[mid] == 2.0f && xy[mid + 1] == -1.0f && zw[mid] == 0.0f && zw[mid + 1] == 1.0f);
    bool all_written = true;
    for (float v : zw) all_written = all_written && v != 99.0f;
    CHECK(all_written);

    std::vector<uint8_t> out((size_t)w * h * 4, 0), mask((size_t)w * h, 9);
    CHECK(ref_interpolate(prev.data(), curr.data(), xy.data(), w, h, 0.3f, out.data(), mask.data(), 0, 0, w, h, 2) == 0);
    bool mask_written = true;
    for (uint8_t m : mask) mask_written = mask_written && m <= 1;
    CHECK(mask_written);
    std::vector<float> still((size_t)w * h * 2, 0.0f);
    CHECK(ref_interpolate(prev.data(), prev.data(), still.data(), w, h, 0.5f, out.data(), nullptr, 0, 0, w, h, 1) == 0);
    int far_off = 0;                                     // zero vectors, both frames the same: the frame itself, up to the
    for (size_t i = 0; i < out.size(); i++)              // resampling at centres that fp32 misses
        far_off += std::abs((int)out[i] - (int)prev[i]) > 1;
    CHECK(far_off == 0);
}
#endif

}  // namespace

int main() {
    conversions();
    common_functions();
    relational();
    fetches();
    stores();
#ifdef LFG_HAVE_REF_SHADERS
    shaders();
#endif
    if (failures) { std::printf("%d of %d checks failed\n", failures, checks); return 1; }
    std::printf("ok %d\n", checks);
    return 0;
}
