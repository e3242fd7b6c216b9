// glsl_shim.hpp -- the GLSL 4.50 built-ins the reference's three compute shaders use, as C++ on the CPU.
//
// TEST INFRASTRUCTURE ONLY, like everything under oracle/.  This header is this project's own code, written from the GLSL 4.50
// and Vulkan 1.3 specifications with the standard library alone; it holds no shader text.  oracle/ref_recipe.py turns the
// reference's shaders/*.comp into C++ with five mechanical edits and compiles them against it (oracle/_ref/, never committed),
// so that the shader text itself runs and oracle/lfg_oracle.c -- a hand restatement of that text -- can be held to it.
//
// What a GLSL implementation may choose is chosen here exactly as lfg_oracle.c's header states it in writing, and each place
// cites that list by number:
//   (1) UNORM8 texel -> float = (float)byte / 255.0f
//   (2) float -> UNORM8 store = clamp to [0, 1] (NaN -> 0), * 255.0f, round half to even
//   (3) LINEAR / CLAMP_TO_EDGE sampler = Vulkan-spec bilinear with fp32 weights, in the oracle's operation order
//   (4) sin = (float)sin((double)x), sqrt = IEEE sqrtf, no contraction (compile with -ffp-contract=off, never -ffast-math)
//   (5) texelFetch outside the image returns (0, 0, 0, 0)
//   (6) fp32 sums in source order, left to right
//   (7) distance(a, b) = sqrt(((dx*dx + dy*dy) + dz*dz) + dw*dw)
//   (9) mix(x, y, a) = x*(1 - a) + y*a
// Choice (8) -- "texture(motionVectors, uv) at an exact texel centre returns that texel" -- is NOT implemented: texture() on a
// vector image is the same choice-(3) bilinear as on a frame, which is how the reference's host code sets that sampler up
// (LINEAR, CLAMP_TO_EDGE, normalised coordinates).  Instead the shim reports where (8) is an assumption: a sampler with
// `report_fraction` set raises the thread's `texture_fraction_seen` whenever a fetch through it had a non-zero fractional
// weight, and the driver collects that per invocation.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

namespace glsl {

// ---------------------------------------------------------------------------------------------------------------- vectors
struct bvec2 { bool x, y; };
struct uvec2 { unsigned x, y; };
struct ivec2;

struct vec2 {
    float x, y;
    vec2() = default;
    explicit vec2(float s) : x(s), y(s) {}
    vec2(float x_, float y_) : x(x_), y(y_) {}
    explicit vec2(const ivec2 &v);                       // int -> float: exact for every image coordinate
};

struct ivec2 {
    int x, y;
    ivec2() = default;
    explicit ivec2(int s) : x(s), y(s) {}
    ivec2(int x_, int y_) : x(x_), y(y_) {}
    explicit ivec2(const uvec2 &v) : x((int)v.x), y((int)v.y) {}
    explicit ivec2(const vec2 &v) : x((int)v.x), y((int)v.y) {}      // GLSL 4.50 5.4.1: float -> int drops the fraction
};

inline vec2::vec2(const ivec2 &v) : x((float)v.x), y((float)v.y) {}

// `.xy` is a data member in GLSL's spelling, so it has to be one here: the two views of a vector share storage through an
// anonymous union, which g++ and clang++ define (a documented extension; both are trivially copyable floats / unsigneds).
struct uvec3 {
    union { struct { unsigned x, y, z; }; uvec2 xy; };
    uvec3() : x(0), y(0), z(0) {}
    uvec3(unsigned x_, unsigned y_, unsigned z_) : x(x_), y(y_), z(z_) {}
};

struct vec4 {
    union { struct { float x, y, z, w; }; vec2 xy; };
    vec4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
    explicit vec4(float s) : x(s), y(s), z(s), w(s) {}
    vec4(float x_, float y_, float z_, float w_) : x(x_), y(y_), z(z_), w(w_) {}
    vec4(const vec2 &v, float z_, float w_) : x(v.x), y(v.y), z(z_), w(w_) {}
    vec4 &operator+=(const vec4 &o) { x += o.x; y += o.y; z += o.z; w += o.w; return *this; }
};

// component-wise operators, each one fp32 operation per component (4), (6)
inline vec2 operator+(vec2 a, vec2 b) { return vec2(a.x + b.x, a.y + b.y); }
inline vec2 operator+(vec2 a, float s) { return vec2(a.x + s, a.y + s); }
inline vec2 operator-(vec2 a, vec2 b) { return vec2(a.x - b.x, a.y - b.y); }
inline vec2 operator-(vec2 a, float s) { return vec2(a.x - s, a.y - s); }
inline vec2 operator*(vec2 a, vec2 b) { return vec2(a.x * b.x, a.y * b.y); }
inline vec2 operator*(vec2 a, float s) { return vec2(a.x * s, a.y * s); }
inline vec2 operator/(vec2 a, vec2 b) { return vec2(a.x / b.x, a.y / b.y); }
inline vec2 operator/(float s, vec2 b) { return vec2(s / b.x, s / b.y); }
inline ivec2 operator+(ivec2 a, ivec2 b) { return ivec2(a.x + b.x, a.y + b.y); }
inline ivec2 operator-(ivec2 a, ivec2 b) { return ivec2(a.x - b.x, a.y - b.y); }
inline vec4 operator*(vec4 a, float s) { return vec4(a.x * s, a.y * s, a.z * s, a.w * s); }
inline vec4 operator/(vec4 a, float s) { return vec4(a.x / s, a.y / s, a.z / s, a.w / s); }
inline vec4 operator+(vec4 a, vec4 b) { return vec4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
inline vec4 operator-(vec4 a, vec4 b) { return vec4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w); }

// ------------------------------------------------------------------------------------------------- relational, GLSL 8.7
inline bool any(bvec2 b) { return b.x || b.y; }
inline bvec2 lessThan(vec2 a, vec2 b) { return bvec2{a.x < b.x, a.y < b.y}; }
inline bvec2 lessThan(ivec2 a, ivec2 b) { return bvec2{a.x < b.x, a.y < b.y}; }
inline bvec2 greaterThan(vec2 a, vec2 b) { return bvec2{a.x > b.x, a.y > b.y}; }
inline bvec2 greaterThan(ivec2 a, ivec2 b) { return bvec2{a.x > b.x, a.y > b.y}; }
inline bvec2 greaterThanEqual(vec2 a, vec2 b) { return bvec2{a.x >= b.x, a.y >= b.y}; }
inline bvec2 greaterThanEqual(ivec2 a, ivec2 b) { return bvec2{a.x >= b.x, a.y >= b.y}; }

// ---------------------------------------------------------------------------------- common and geometric, GLSL 8.1 - 8.5
inline float floor(float x) { return std::floor(x); }
inline vec2 floor(vec2 v) { return vec2(std::floor(v.x), std::floor(v.y)); }
inline float fract(float x) { return x - std::floor(x); }                                 // GLSL 8.3: x - floor(x)
inline vec2 fract(vec2 v) { return vec2(fract(v.x), fract(v.y)); }
inline float sin(float x) { return (float)std::sin((double)x); }                          // (4)
inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }            // (9)
inline vec4 mix(vec4 x, vec4 y, float a) { return vec4(mix(x.x, y.x, a), mix(x.y, y.y, a), mix(x.z, y.z, a), mix(x.w, y.w, a)); }
inline float distance(vec4 p, vec4 q) {                                                    // (7), (4)
    const vec4 d = p - q;
    return std::sqrt(((d.x * d.x + d.y * d.y) + d.z * d.z) + d.w * d.w);
}

// ------------------------------------------------------------------------------------------------------ images and samplers
// Both are views of caller memory, tightly packed and row-major.  RGBA8 is four UNORM bytes per texel.  RG32F_OF_RGBA32F is
// the .xy of an rgba32f image, two floats per texel: a fetch supplies z = 0 and w = 1 -- what motion.comp stores there -- and a
// store writes .xy to `data` and, where the caller gave one, .zw to `zw`.
enum class Format { RGBA8, RG32F_OF_RGBA32F };

struct sampler2D {
    const void *data = nullptr;
    int width = 0, height = 0;
    Format format = Format::RGBA8;
    bool report_fraction = false;
};

struct image2D {
    void *data = nullptr;
    float *zw = nullptr;
    int width = 0, height = 0;
    Format format = Format::RGBA8;
    int x0 = 0, y0 = 0, x1 = 0, y1 = 0;                  // the driver's store window: what the caller asked to have written
};

inline thread_local uvec3 gl_GlobalInvocationID;
inline thread_local bool texture_fraction_seen = false;

inline vec4 load_texel(const sampler2D &s, int x, int y) {
    const size_t at = (size_t)y * (size_t)s.width + (size_t)x;
    if (s.format == Format::RGBA8) {
        const uint8_t *p = (const uint8_t *)s.data + at * 4u;
        return vec4((float)p[0] / 255.0f, (float)p[1] / 255.0f, (float)p[2] / 255.0f, (float)p[3] / 255.0f);   // (1)
    }
    const float *p = (const float *)s.data + at * 2u;
    return vec4(p[0], p[1], 0.0f, 1.0f);
}

inline vec4 texelFetch(const sampler2D &s, ivec2 p, int /*lod*/) {
    if (p.x < 0 || p.y < 0 || p.x >= s.width || p.y >= s.height) return vec4(0.0f);       // (5)
    return load_texel(s, p.x, p.y);
}

inline int clamp_index(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// (3): Vulkan 1.3 section 16.6 (unnormalise, i0 = floor(u - 0.5), fraction as the weight) and 16.9.1's linear sum, with
// CLAMP_TO_EDGE applied per index, in fp32 and in the oracle's order of operations.  The same code serves a frame and a
// vector image: choice (8) is deliberately absent.
inline vec4 texture(const sampler2D &s, vec2 uv) {
    const float u = uv.x * (float)s.width - 0.5f, v = uv.y * (float)s.height - 0.5f;
    const float fu = std::floor(u), fv = std::floor(v);
    const float a = u - fu, b = v - fv;
    if (s.report_fraction && (a != 0.0f || b != 0.0f)) texture_fraction_seen = true;
    const int i0 = clamp_index((int)fu, s.width - 1), i1 = clamp_index((int)fu + 1, s.width - 1);
    const int j0 = clamp_index((int)fv, s.height - 1), j1 = clamp_index((int)fv + 1, s.height - 1);
    const vec4 t00 = load_texel(s, i0, j0), t10 = load_texel(s, i1, j0), t01 = load_texel(s, i0, j1), t11 = load_texel(s, i1, j1);
    const float w00 = (1.0f - a) * (1.0f - b), w10 = a * (1.0f - b), w01 = (1.0f - a) * b, w11 = a * b;
    return vec4(((w00 * t00.x + w10 * t10.x) + w01 * t01.x) + w11 * t11.x,               // (6)
                ((w00 * t00.y + w10 * t10.y) + w01 * t01.y) + w11 * t11.y,
                ((w00 * t00.z + w10 * t10.z) + w01 * t01.z) + w11 * t11.z,
                ((w00 * t00.w + w10 * t10.w) + w01 * t01.w) + w11 * t11.w);
}

inline uint8_t to_unorm8(float v) {                                                         // (2)
    if (!(v > 0.0f)) v = 0.0f;                           // NaN and everything below 0
    if (v > 1.0f) v = 1.0f;
    return (uint8_t)std::lrint(v * 255.0f);              // the default rounding mode: half to even
}

// A store outside the image has no effect (GLSL 4.50 section 8.12); one outside the driver's window is dropped as well.
inline void imageStore(const image2D &img, ivec2 p, vec4 c) {
    if (p.x < 0 || p.y < 0 || p.x >= img.width || p.y >= img.height) return;
    if (p.x < img.x0 || p.y < img.y0 || p.x >= img.x1 || p.y >= img.y1) return;
    const size_t at = (size_t)p.y * (size_t)img.width + (size_t)p.x;
    if (img.format == Format::RGBA8) {
        uint8_t *o = (uint8_t *)img.data + at * 4u;
        o[0] = to_unorm8(c.x); o[1] = to_unorm8(c.y); o[2] = to_unorm8(c.z); o[3] = to_unorm8(c.w);
        return;
    }
    float *o = (float *)img.data + at * 2u;
    o[0] = c.x; o[1] = c.y;
    if (img.zw) { img.zw[at * 2u] = c.z; img.zw[at * 2u + 1u] = c.w; }
}

}  // namespace glsl

// What a generated file says once inside its own namespace.  sin and floor are declared by name so that they hide the C
// library's ::sin and ::floor, which a using-directive alone would leave as equally good candidates.
#define GLSL_SHIM_NAMES using namespace glsl; using glsl::sin; using glsl::floor;
