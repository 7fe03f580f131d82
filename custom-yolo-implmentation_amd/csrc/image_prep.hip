// On-device input pipeline: the reference's training transform
//   ToImage -> RandomHorizontalFlip -> Resize((S, S)) -> ColorJitter(brightness, contrast, saturation, hue) ->
//   ToDtype(float32, scale=True) -> Normalize(mean, std)                       (src/data/transforms.py:4-14)
// for a whole batch of decoded uint8 HWC images of different sizes, with the random decisions (flip, the four jitter
// factors and their order) drawn on the host and passed in.  torchvision is not in this image (parity unpinned for
// its arithmetic); the kernels follow torchvision.transforms.v2.functional 0.24 as published:
//   resize        bilinear with antialiasing = torch's _upsample_bilinear2d_aa: separable triangle filter whose support
//                 is the scale factor when shrinking, accumulated in fp32 and rounded to uint8 (the reference resizes
//                 the uint8 image; its fixed-point two-pass form may differ from this by one level)
//   brightness    blend(img, 0, f)            = trunc(clamp(img * f, 0, 255))
//   contrast      blend(img, mean(floor(gray)), f),  gray = 0.2989 R + 0.587 G + 0.114 B
//   saturation    blend(img, floor(gray), f)
//   hue           RGB/255 -> HSV, h = (h + f) mod 1, -> RGB, -> uint8 by floor(x * (256 - 1e-3))
//   to float      x / 255, (x - mean) / std
// Stages: resize+flip -> uint8 planar staging; per jitter slot k = 0..3 a per-image gray-mean reduction and the op that
// image has in slot k; the last launch converts, normalises and writes NCHW in the model's input dtype.
// Mosaic (no reference counterpart; opt-in): k_mosaic takes the place of the resize launch and composes each output from
// four resized tiles of the batch's own images around a centre, fill elsewhere; the colour chain behind it is the same.
// Affine warp (no reference counterpart; opt-in): k_affine gathers the finished canvas of the resize or mosaic launch through
// an inverse 2x3 matrix, bilinear with a constant `fill` border, into a second staging buffer; the colour chain runs on that.
// MixUp (no reference counterpart; opt-in): k_mixup blends the finished canvas of an output with the finished, unmixed canvas of
// another output of the same batch, streaming from one staging buffer into the other; the colour chain runs on the mixed one.
// Letterbox (no reference counterpart; the inference interface `Model.predict`): k_letterbox resizes each source to an integer
// rectangle inside the canvas, fills the bars and writes the normalised NCHW input in the same launch -- no staging buffer.
#include "common.h"
#include "letter_rec.h"

struct PrepImage {
    long off;           // byte offset of the image (uint8 HWC, row stride W*3) in the source buffer
    int H, W;
    int flip;
    int order[4];       // op in jitter slot k: 0 brightness, 1 contrast, 2 saturation, 3 hue, -1 none
    float factor[4];    // factor of op o (indexed by op, not by slot)
};

// one of the four tiles of a mosaic output (tile k touches the centre (cx, cy) with one corner: 0 top-left, 1 top-right,
// 2 bottom-left, 3 bottom-right): the source image resized to (th, tw) and placed with its top-left corner at (x0, y0)
struct MosaicTile {
    long off;           // byte offset of the source image in the source buffer
    int H, W;
    int flip;
    int tw, th;         // size of the resized tile; 0 = no tile (the quadrant is fill)
    int x0, y0;         // canvas position of the tile's pixel (0, 0); may be negative (the quadrant clips the tile)
    int cx, cy;         // the output's centre, repeated in its four tiles
};

// the inverse map of one output's warp, canvas <- output, in continuous coordinates (pixel i covers [i, i + 1)): the six fp32
// values the host rounded once from the float64 inverse of the forward matrix
struct AffineRec { float a00, a01, b0, a10, a11, b1; };

// the mix of one output: the output of the same batch whose finished, unmixed canvas is blended in, and the share r of the
// output's own canvas; partner = the output's own index means "not mixed" (a copy: no partner is read)
struct MixRec { int partner; float r; };

namespace {

__device__ __forceinline__ float tri(float x) { x = fabsf(x); return x < 1.f ? 1.f - x : 0.f; }

// weights of output index i along one axis (torch aten/src/ATen/native/cpu/UpSampleKernel.cpp, antialias bilinear)
struct Taps { int lo, n; float scale, inv, center; };
__device__ __forceinline__ Taps taps_of(int i, int in_size, int out_size) {
    Taps t;
    t.scale = (float)in_size / (float)out_size;
    const float support = t.scale >= 1.f ? t.scale : 1.f;
    t.inv = t.scale >= 1.f ? 1.f / t.scale : 1.f;
    t.center = t.scale * ((float)i + 0.5f);
    t.lo = max(0, (int)(t.center - support + 0.5f));
    t.n = min(in_size, (int)(t.center + support + 0.5f)) - t.lo;
    return t;
}

// output pixel (oy, ox) of the image at `base` (uint8 HWC, H x W, optionally mirrored) resized to (out_h, out_w): all three
// channels, rounded to uint8 levels.  The one pixel routine of k_resize_flip and k_mosaic: the same operations in the same
// order for both (this file is compiled without floating-point contraction), so a mosaic record that describes a plain
// resize reproduces k_resize_flip bit for bit.  Reads stay inside [0, H) x [0, W) by the clamping in taps_of.
__device__ __forceinline__ void resize_pixel(const unsigned char* __restrict__ base, int H, int W, int flip, int oy, int ox,
                                             int out_h, int out_w, unsigned char px[3]) {
    const Taps ty = taps_of(oy, H, out_h), tx = taps_of(ox, W, out_w);
    float wsum_y = 0.f, wsum_x = 0.f;
    for (int j = 0; j < ty.n; ++j) wsum_y += tri(((float)(j + ty.lo) - ty.center + 0.5f) * ty.inv);
    for (int j = 0; j < tx.n; ++j) wsum_x += tri(((float)(j + tx.lo) - tx.center + 0.5f) * tx.inv);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int jy = 0; jy < ty.n; ++jy) {
        const float wy = tri(((float)(jy + ty.lo) - ty.center + 0.5f) * ty.inv) / wsum_y;
        const unsigned char* row = base + (long)(ty.lo + jy) * W * 3;
        float r[3] = {0.f, 0.f, 0.f};
        for (int jx = 0; jx < tx.n; ++jx) {
            const float wx = tri(((float)(jx + tx.lo) - tx.center + 0.5f) * tx.inv);
            const int sx = tx.lo + jx;
            const unsigned char* p = row + (long)(flip ? W - 1 - sx : sx) * 3;
            r[0] += wx * (float)p[0]; r[1] += wx * (float)p[1]; r[2] += wx * (float)p[2];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wy * r[c] / wsum_x;
    }
    // a flipped image is resized from the flipped source: output column ox reads mirrored columns, i.e. the same
    // result as flipping first (the filter is symmetric); written at ox
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = (unsigned char)fminf(fmaxf(floorf(acc[c] + 0.5f), 0.f), 255.f);
}

// one thread per output pixel: all three channels
__global__ __launch_bounds__(256) void k_resize_flip(const unsigned char* __restrict__ src, const PrepImage* __restrict__ imgs,
                                                    unsigned char* __restrict__ stage, int S) {
    const int n = blockIdx.z;
    const PrepImage im = imgs[n];
    const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (ox >= S) return;
    unsigned char px[3];
    resize_pixel(src + im.off, im.H, im.W, im.flip, oy, ox, S, S, px);
#pragma unroll
    for (int c = 0; c < 3; ++c) stage[(((long)n * 3 + c) * S + oy) * S + ox] = px[c];
}

// mosaic: one thread per canvas pixel, four tile records per output image.  The pixel belongs to the quadrant its side of
// the centre says; inside that quadrant's tile rectangle it is the tile's resized pixel, elsewhere the fill level (no
// taps are computed there).  A tile with tw = 0 (an unreachable quadrant of a plain record) is never sampled.
__global__ __launch_bounds__(256) void k_mosaic(const unsigned char* __restrict__ src, const MosaicTile* __restrict__ tiles,
                                               unsigned char* __restrict__ stage, int S, int fill) {
    const int n = blockIdx.z;
    const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (ox >= S) return;
    const MosaicTile* quad = tiles + (long)n * 4;
    const int k = (ox >= quad[0].cx ? 1 : 0) + (oy >= quad[0].cy ? 2 : 0);
    const MosaicTile t = quad[k];
    const int lx = ox - t.x0, ly = oy - t.y0;
    unsigned char px[3] = {(unsigned char)fill, (unsigned char)fill, (unsigned char)fill};
    if (lx >= 0 && lx < t.tw && ly >= 0 && ly < t.th) resize_pixel(src + t.off, t.H, t.W, t.flip, ly, lx, t.th, t.tw, px);
#pragma unroll
    for (int c = 0; c < 3; ++c) stage[(((long)n * 3 + c) * S + oy) * S + ox] = px[c];
}

// affine warp: one thread per output pixel, all three channels; 32 x 8 pixels per workgroup, so that a rotated workgroup
// reads a compact patch of the canvas.  Operation order (every operation rounds once; no contraction in this file):
//   px = ox + 0.5f, py = oy + 0.5f;  u = ((a00 * px + a01 * py) + b0) - 0.5f;  v = ((a10 * px + a11 * py) + b1) - 0.5f
//   u or v outside [-1, S) (tested in float; a NaN fails it too): all four taps lie outside, the pixel is `fill`, nothing is
//   read and no float is converted to int
//   x0 = floor(u), fx = u - x0 (y likewise), so x0 in [-1, S - 1]; a tap with an index outside [0, S) is `fill`, every load
//   is therefore inside the canvas
//   top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10), acc = top + fy * (bot - top): fx = fy = 0 gives p00 itself
//   level = clamp(floor(acc + 0.5f), 0, 255), as resize_pixel quantises
__global__ __launch_bounds__(256) void k_affine(const unsigned char* __restrict__ stage, const AffineRec* __restrict__ recs,
                                               unsigned char* __restrict__ stage2, int S, int fill) {
    const int n = blockIdx.z;
    const int ox = blockIdx.x * 32 + (threadIdx.x & 31), oy = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (ox >= S || oy >= S) return;
    const AffineRec A = recs[n];
    const float px = (float)ox + 0.5f, py = (float)oy + 0.5f;
    const float u = ((A.a00 * px + A.a01 * py) + A.b0) - 0.5f;
    const float v = ((A.a10 * px + A.a11 * py) + A.b1) - 0.5f;
    const float ff = (float)fill, fs = (float)S;
    const long hw = (long)S * S;
    float acc[3] = {ff, ff, ff};
    if (u >= -1.f && u < fs && v >= -1.f && v < fs) {
        const float xf = floorf(u), yf = floorf(v);
        const float fx = u - xf, fy = v - yf;
        const int x0 = (int)xf, y0 = (int)yf;                 // in [-1, S - 1] by the test above
        const bool l = x0 >= 0, r = x0 + 1 < S, t = y0 >= 0, b = y0 + 1 < S;
        const unsigned char* base = stage + (long)n * 3 * hw;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned char* pl = base + c * hw;
            const float p00 = (t && l) ? (float)pl[(long)y0 * S + x0] : ff;
            const float p01 = (t && r) ? (float)pl[(long)y0 * S + x0 + 1] : ff;
            const float p10 = (b && l) ? (float)pl[(long)(y0 + 1) * S + x0] : ff;
            const float p11 = (b && r) ? (float)pl[(long)(y0 + 1) * S + x0 + 1] : ff;
            const float top = p00 + fx * (p01 - p00), bot = p10 + fx * (p11 - p10);
            acc[c] = top + fy * (bot - top);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c)
        stage2[(long)n * 3 * hw + c * hw + (long)oy * S + ox] = (unsigned char)fminf(fmaxf(floorf(acc[c] + 0.5f), 0.f), 255.f);
}

// one mixed level.  Operation order (every operation rounds once; no contraction in this file):
//   level = clamp(floor((r * a + q * b) + 0.5f), 0, 255) with q = 1.0f - r, as resize_pixel quantises
// r = 1 gives 1 * a + 0 * b = a and r = 0 gives b, exactly
__device__ __forceinline__ unsigned mix_level(unsigned a, unsigned b, float r, float q) {
    return (unsigned)fminf(fmaxf(floorf((r * (float)a + q * (float)b) + 0.5f), 0.f), 255.f);
}

__device__ __forceinline__ unsigned mix_word(unsigned a, unsigned b, float r, float q) {     // four levels of one dword
    unsigned o = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) o |= mix_level((a >> k) & 255u, (b >> k) & 255u, r, q) << k;
    return o;
}

// mixup: output n = r * (canvas n) + (1 - r) * (canvas of its partner), a stream over the B = 3 S^2 bytes of every image
// from `in` (the finished, unmixed canvases) to `out` (another buffer: two outputs that choose each other both read unmixed
// canvases).  blockIdx.y is the image, so the record is one load per workgroup and "no partner" (partner == n: a copy that
// reads nothing else) is a uniform branch.  V = 16: one 16-byte vector per lane from each canvas and one store; the host takes
// it when B % 16 == 0 and both buffers are 16-byte aligned, so that every image base is.  V = 1 otherwise: the same levels
template <int V>
__global__ __launch_bounds__(256) void k_mixup(const unsigned char* __restrict__ in, const MixRec* __restrict__ recs,
                                              unsigned char* __restrict__ out, long B) {
    const int n = blockIdx.y;
    const MixRec m = recs[n];
    const long i = ((long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i >= B) return;                                            // B % V == 0: a lane's V bytes are all inside or all outside
    const unsigned char* a = in + (long)n * B + i;
    const unsigned char* b = in + (long)m.partner * B + i;
    unsigned char* o = out + (long)n * B + i;
    const float r = m.r, q = 1.0f - m.r;
    if (V == 16) {
        uint4 va = *(const uint4*)a;
        if (m.partner != n) {
            const uint4 vb = *(const uint4*)b;
            va.x = mix_word(va.x, vb.x, r, q); va.y = mix_word(va.y, vb.y, r, q);
            va.z = mix_word(va.z, vb.z, r, q); va.w = mix_word(va.w, vb.w, r, q);
        }
        *(uint4*)o = va;
    } else {
        *o = m.partner != n ? (unsigned char)mix_level(*a, *b, r, q) : *a;
    }
}

__device__ __forceinline__ float gray_of(float r, float g, float b) { return floorf(0.2989f * r + 0.587f * g + 0.114f * b); }

// mean of floor(gray) per image -> means[n] (fp32, zeroed by the caller); one block row per image
__global__ __launch_bounds__(256) void k_gray_mean(const unsigned char* __restrict__ stage, int S, float* __restrict__ means) {
    const int n = blockIdx.y;
    const long hw = (long)S * S;
    const unsigned char* r = stage + (long)n * 3 * hw;
    float acc = 0.f;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < hw; i += (long)gridDim.x * blockDim.x)
        acc += gray_of((float)r[i], (float)r[hw + i], (float)r[2 * hw + i]);
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) atomicAdd(means + n, acc / (float)hw);
}

__device__ __forceinline__ float blend_u8(float a, float b, float ratio) {      // trunc(clamp(a*ratio + b*(1-ratio)))
    return floorf(fminf(fmaxf(a * ratio + b * (1.f - ratio), 0.f), 255.f));
}

__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float f) {
    // torchvision _rgb_to_hsv / _hsv_to_rgb on [0,1] floats
    r *= (1.f / 255.f); g *= (1.f / 255.f); b *= (1.f / 255.f);
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.f : maxc);
    const float crd = eqc ? 1.f : cr;
    const float rc = (maxc - r) / crd, gc = (maxc - g) / crd, bc = (maxc - b) / crd;
    const float hr = maxc == r ? bc - gc : 0.f;
    const float hg = (maxc == g && maxc != r) ? 2.f + rc - bc : 0.f;
    const float hb = (maxc != g && maxc != r) ? 4.f + gc - rc : 0.f;
    float h = fmodf((hr + hg + hb) / 6.f + 1.f, 1.f);
    h = h + f;
    h = h - floorf(h);                                       // remainder(1.0)
    const float v = maxc;
    const float h6 = h * 6.f;
    const float fi = floorf(h6);
    const float ff = h6 - fi;
    const int i = ((int)fi) % 6;
    const float p = fminf(fmaxf(v * (1.f - s), 0.f), 1.f), q = fminf(fmaxf(v * (1.f - s * ff), 0.f), 1.f);
    const float t = fminf(fmaxf(v * (1.f - s * (1.f - ff)), 0.f), 1.f);
    float ro, go, bo;
    switch (i) {
        case 0: ro = v; go = t; bo = p; break;
        case 1: ro = q; go = v; bo = p; break;
        case 2: ro = p; go = v; bo = t; break;
        case 3: ro = p; go = q; bo = v; break;
        case 4: ro = t; go = p; bo = v; break;
        default: ro = v; go = p; bo = q; break;
    }
    const float k = 255.f + 1.f - 1e-3f;                     // float -> uint8 of to_dtype(scale=True)
    r = floorf(ro * k); g = floorf(go * k); b = floorf(bo * k);
}

// jitter slot `slot` of every image, in place on the staging buffer; FINAL: instead write (x/255 - mean)/std as T NCHW
template <typename T, bool FINAL>
__global__ __launch_bounds__(256) void k_color(unsigned char* __restrict__ stage, const PrepImage* __restrict__ imgs, int slot,
                                               const float* __restrict__ means, int S, T* __restrict__ out, float m0, float m1,
                                               float m2, float s0, float s1, float s2) {
    const int n = blockIdx.y;
    const PrepImage im = imgs[n];
    const int op = slot >= 0 ? im.order[slot] : -1;
    const float f = op >= 0 ? im.factor[op] : 1.f;
    const float mean = means != nullptr ? means[n] : 0.f;
    const long hw = (long)S * S;
    unsigned char* base = stage + (long)n * 3 * hw;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < hw; i += (long)gridDim.x * blockDim.x) {
        float r = (float)base[i], g = (float)base[hw + i], b = (float)base[2 * hw + i];
        if (op == 0) { r = blend_u8(r, 0.f, f); g = blend_u8(g, 0.f, f); b = blend_u8(b, 0.f, f); }
        else if (op == 1) { r = blend_u8(r, mean, f); g = blend_u8(g, mean, f); b = blend_u8(b, mean, f); }
        else if (op == 2) { const float gr = gray_of(r, g, b); r = blend_u8(r, gr, f); g = blend_u8(g, gr, f); b = blend_u8(b, gr, f); }
        else if (op == 3) hue_shift(r, g, b, f);
        if (FINAL) {
            T* o = out + (long)n * 3 * hw;
            o[i] = from_f<T>((r * (1.f / 255.f) - m0) / s0);
            o[hw + i] = from_f<T>((g * (1.f / 255.f) - m1) / s1);
            o[2 * hw + i] = from_f<T>((b * (1.f / 255.f) - m2) / s2);
        } else {
            base[i] = (unsigned char)r; base[hw + i] = (unsigned char)g; base[2 * hw + i] = (unsigned char)b;
        }
    }
}

// letterbox: one thread per canvas pixel, straight from the uint8 sources to the model's input.  Inside the record's rectangle
// the three levels are resize_pixel's (the routine of k_resize_flip and k_mosaic), elsewhere `fill`; the conversion is
// k_color<T, true>'s, operation for operation, so the launch reproduces k_mosaic + k_color<T, true> bit for bit.  The grid
// depends on N and S only; the tap loops take their lengths from the record
template <typename T>
__global__ __launch_bounds__(256) void k_letterbox(const unsigned char* __restrict__ src, const LetterRec* __restrict__ recs,
                                                  int S, int fill, T* __restrict__ out, float m0, float m1, float m2, float s0,
                                                  float s1, float s2) {
    const int n = blockIdx.z;
    const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (ox >= S) return;
    const LetterRec L = recs[n];
    const int lx = ox - L.left, ly = oy - L.top;
    unsigned char px[3] = {(unsigned char)fill, (unsigned char)fill, (unsigned char)fill};
    if (lx >= 0 && lx < L.nw && ly >= 0 && ly < L.nh) resize_pixel(src + L.off, L.H, L.W, 0, ly, lx, L.nh, L.nw, px);
    const long hw = (long)S * S, i = (long)oy * S + ox;
    T* o = out + (long)n * 3 * hw;
    o[i] = from_f<T>(((float)px[0] * (1.f / 255.f) - m0) / s0);
    o[hw + i] = from_f<T>(((float)px[1] * (1.f / 255.f) - m1) / s1);
    o[2 * hw + i] = from_f<T>(((float)px[2] * (1.f / 255.f) - m2) / s2);
}

}  // namespace

extern "C" {

int yolo_letter_bytes(void) { return (int)sizeof(LetterRec); }

// fill record `index` of the host-side letterbox table of a launch on an S x S canvas over a source buffer of `src_bytes`
// bytes.  Refused: an image that does not lie inside the buffer, a rectangle that leaves the canvas, exactly one of nw, nh
// being 0, a scale that is not finite and positive (a NaN fails the comparison) -- so every device read lies inside the
// source buffer.  nw = nh = 0: the blank slot (H, W >= 0, nothing is read)
int yolo_letter_fill(void* table_host, int index, long off, int H, int W, int nw, int nh, int left, int top, float sx, float sy,
                     int S, long src_bytes) {
    if (table_host == nullptr || index < 0 || S <= 0 || off < 0 || off > src_bytes || H < 0 || W < 0) return YOLO_ERR_ARG;
    if ((long)H * W > (src_bytes - off) / 3) return YOLO_ERR_ARG;                 // off + 3 H W > src_bytes, without overflow
    if (nw < 0 || nw > S || nh < 0 || nh > S || (nw == 0) != (nh == 0)) return YOLO_ERR_ARG;
    if (nw > 0 && (H <= 0 || W <= 0)) return YOLO_ERR_ARG;
    if (left < 0 || top < 0 || left > S - nw || top > S - nh) return YOLO_ERR_ARG;
    if (!(sx > 0.f && sx - sx == 0.f && sy > 0.f && sy - sy == 0.f)) return YOLO_ERR_ARG;
    LetterRec& r = ((LetterRec*)table_host)[index];
    r.off = off; r.H = H; r.W = W; r.nw = nw; r.nh = nh; r.left = left; r.top = top; r.sx = sx; r.sy = sy;
    return YOLO_OK;
}

int yolo_prep_image_bytes(void) { return (int)sizeof(PrepImage); }

// fill record `index` of the host-side table (order[k] = op of jitter slot k or -1; factor indexed by op)
int yolo_prep_image_fill(void* table_host, int index, long off, int H, int W, int flip, int o0, int o1, int o2, int o3,
                         float brightness, float contrast, float saturation, float hue) {
    if (H <= 0 || W <= 0) return YOLO_ERR_ARG;
    PrepImage& p = ((PrepImage*)table_host)[index];
    p.off = off; p.H = H; p.W = W; p.flip = flip;
    p.order[0] = o0; p.order[1] = o1; p.order[2] = o2; p.order[3] = o3;
    p.factor[0] = brightness; p.factor[1] = contrast; p.factor[2] = saturation; p.factor[3] = hue;
    return YOLO_OK;
}

int yolo_mosaic_tile_bytes(void) { return (int)sizeof(MosaicTile); }

// fill tile `tile` (0..3) of output `image` in the host-side tile table ([N][4] records, zeroed by the caller: a tile left
// zeroed is all fill)
int yolo_mosaic_tile_fill(void* table_host, int image, int tile, long off, int H, int W, int flip, int tw, int th, int x0, int y0,
                          int cx, int cy) {
    if (H <= 0 || W <= 0 || tw <= 0 || th <= 0 || tile < 0 || tile > 3 || image < 0) return YOLO_ERR_ARG;
    MosaicTile& t = ((MosaicTile*)table_host)[(long)image * 4 + tile];
    t.off = off; t.H = H; t.W = W; t.flip = flip; t.tw = tw; t.th = th; t.x0 = x0; t.y0 = y0; t.cx = cx; t.cy = cy;
    return YOLO_OK;
}

int yolo_affine_bytes(void) { return (int)sizeof(AffineRec); }

// fill record `index` of the host-side affine table: the inverse map (canvas <- output), finite values only
int yolo_affine_fill(void* table_host, int index, float a00, float a01, float b0, float a10, float a11, float b1) {
    const float v[6] = {a00, a01, b0, a10, a11, b1};
    for (int k = 0; k < 6; ++k)
        if (!(v[k] - v[k] == 0.f)) return YOLO_ERR_ARG;       // inf - inf and nan - nan are nan
    if (index < 0) return YOLO_ERR_ARG;
    AffineRec& a = ((AffineRec*)table_host)[index];
    a.a00 = a00; a.a01 = a01; a.b0 = b0; a.a10 = a10; a.a11 = a11; a.b1 = b1;
    return YOLO_OK;
}

int yolo_mix_bytes(void) { return (int)sizeof(MixRec); }

// fill record `index` of the host-side mix table of a batch of N outputs: partner inside the batch (partner == index: not
// mixed), r finite and in [0, 1] (a NaN fails both comparisons)
int yolo_mix_fill(void* table_host, int index, int partner, float r, int N) {
    if (index < 0 || index >= N || partner < 0 || partner >= N || !(r >= 0.f && r <= 1.f)) return YOLO_ERR_ARG;
    MixRec& m = ((MixRec*)table_host)[index];
    m.partner = partner; m.r = r;
    return YOLO_OK;
}

}  // extern "C"

// the colour chain on the staging buffer: per jitter slot a gray-mean reduction and that slot's op, the last launch
// converts, normalises and writes NCHW (jitter = 0: that last launch alone)
static int color_chain(const PrepImage* imgs, int N, int S, int jitter, void* stage, float* means, void* out, int out_dtype,
                       float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t st) {
    const long hw = (long)S * S;
    int gx = (int)((hw + 255) / 256);
    if (gx > 64) gx = 64;
    if (jitter) {
        int rc = yolo_zero_async(means, (size_t)4 * N * sizeof(float), st);
        if (rc) return rc;
    }
    const int nslot = jitter ? 4 : 1;
    for (int k = 0; k < nslot; ++k) {
        const int slot = jitter ? k : -1;
        float* mk = jitter ? means + (long)k * N : nullptr;
        if (jitter) hipLaunchKernelGGL(k_gray_mean, dim3(gx, N), dim3(256), 0, st, (const unsigned char*)stage, S, mk);
        if (k + 1 < nslot) {
            hipLaunchKernelGGL((k_color<float, false>), dim3(gx, N), dim3(256), 0, st, (unsigned char*)stage, imgs, slot, mk, S,
                               (float*)nullptr, m0, m1, m2, s0, s1, s2);
        } else {
            YOLO_DISPATCH_T(out_dtype, hipLaunchKernelGGL((k_color<T, true>), dim3(gx, N), dim3(256), 0, st, (unsigned char*)stage,
                                                          imgs, slot, mk, S, (T*)out, m0, m1, m2, s0, s1, s2));
        }
    }
    return YOLO_LAUNCH_CHECK();
}

// the one launch sequence of the four yolo_image_prep* entries (a new stage is added HERE, once): the canvas into `stage` (k_mosaic
// when tiles_dev is given, else k_resize_flip); with affine_dev, k_affine into the other buffer; with mix_dev, k_mixup into the buffer
// that is free by then (the kernel before it has finished reading it: stream order); the colour chain where the finished canvas lies.
// stage2 is not touched when both tables are null.  The entries refuse bad arguments, each its own; nothing is checked here
static int prep_run(const void* src, const void* table_dev, const void* tiles_dev, const void* affine_dev, const void* mix_dev, int N,
                    int S, int fill, int jitter, void* stage, void* stage2, float* means, void* out, int out_dtype, float m0, float m1,
                    float m2, float s0, float s1, float s2, hipStream_t st) {
    const PrepImage* imgs = (const PrepImage*)table_dev;
    const unsigned char* in = (const unsigned char*)src;
    unsigned char *canvas = (unsigned char*)stage, *other = (unsigned char*)stage2;
    const dim3 rows(ceil_div(S, 256), S, N), blk(256);
    if (tiles_dev == nullptr) hipLaunchKernelGGL(k_resize_flip, rows, blk, 0, st, in, imgs, canvas, S);
    else hipLaunchKernelGGL(k_mosaic, rows, blk, 0, st, in, (const MosaicTile*)tiles_dev, canvas, S, fill);
    if (affine_dev != nullptr) {
        hipLaunchKernelGGL(k_affine, dim3(ceil_div(S, 32), ceil_div(S, 8), N), blk, 0, st, canvas, (const AffineRec*)affine_dev, other, S,
                           fill);
        canvas = other; other = (unsigned char*)stage;
    }
    if (mix_dev != nullptr) {
        const long B = 3L * S * S;
        if (B % 16 == 0 && (uintptr_t)canvas % 16 == 0 && (uintptr_t)other % 16 == 0)
            hipLaunchKernelGGL(k_mixup<16>, dim3((unsigned)((B / 16 + 255) / 256), N), blk, 0, st, canvas, (const MixRec*)mix_dev, other, B);
        else
            hipLaunchKernelGGL(k_mixup<1>, dim3((unsigned)((B + 255) / 256), N), blk, 0, st, canvas, (const MixRec*)mix_dev, other, B);
        canvas = other;
    }
    return color_chain(imgs, N, S, jitter, canvas, means, out, out_dtype, m0, m1, m2, s0, s1, s2, st);
}

extern "C" {

// src: all images of the batch, uint8 HWC, back to back (table[i].off); stage: uint8 scratch [N][3][S][S]; means: fp32
// scratch [4][N]; out: [N][3][S][S] of out_dtype.  jitter = 0 skips the colour stages (validation transform).
int yolo_image_prep(const void* src, const void* table_dev, int N, int S, int jitter, void* stage, float* means, void* out,
                    int out_dtype, float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t st) {
    if (N <= 0 || S <= 0) return YOLO_ERR_ARG;
    return prep_run(src, table_dev, nullptr, nullptr, nullptr, N, S, 0, jitter, stage, nullptr, means, out, out_dtype, m0, m1, m2, s0,
                    s1, s2, st);
}

// the same with a mosaic in front of the colour chain: tiles_dev = [N][4] MosaicTile records (yolo_mosaic_tile_fill),
// table_dev = the N PrepImage records, of which only the jitter order / factors of each OUTPUT image are read
int yolo_image_prep_mosaic(const void* src, const void* tiles_dev, const void* table_dev, int N, int S, int fill, int jitter,
                           void* stage, float* means, void* out, int out_dtype, float m0, float m1, float m2, float s0, float s1,
                           float s2, hipStream_t st) {
    if (N <= 0 || S <= 0 || fill < 0 || fill > 255) return YOLO_ERR_ARG;
    return prep_run(src, table_dev, tiles_dev, nullptr, nullptr, N, S, fill, jitter, stage, nullptr, means, out, out_dtype, m0, m1, m2,
                    s0, s1, s2, st);
}

// the same with an affine warp between the canvas and the colour chain: k_affine gathers the canvas through affine_dev ([N]
// yolo_affine_fill records) into stage2 ([N][3][S][S] uint8, not overlapping stage), and the colour chain runs on stage2.  `fill` is
// the level of the mosaic's empty quadrants and of the warp's uncovered pixels
int yolo_image_prep_affine(const void* src, const void* tiles_dev, const void* table_dev, const void* affine_dev, int N, int S,
                           int fill, int jitter, void* stage, void* stage2, float* means, void* out, int out_dtype, float m0,
                           float m1, float m2, float s0, float s1, float s2, hipStream_t st) {
    if (N <= 0 || S <= 0 || fill < 0 || fill > 255 || affine_dev == nullptr || stage2 == nullptr || stage2 == stage)
        return YOLO_ERR_ARG;
    return prep_run(src, table_dev, tiles_dev, affine_dev, nullptr, N, S, fill, jitter, stage, stage2, means, out, out_dtype, m0, m1,
                    m2, s0, s1, s2, st);
}

// the same with a mixup between the finished canvas and the colour chain: tiles_dev = nullptr -> the plain resize, else the mosaic;
// affine_dev = nullptr -> no warp.  mix_dev: [N] yolo_mix_fill records.  Two uint8 stages, always (the chain ends on stage2 without the
// warp, on stage with it)
int yolo_image_prep_mixup(const void* src, const void* tiles_dev, const void* table_dev, const void* affine_dev, const void* mix_dev,
                          int N, int S, int fill, int jitter, void* stage, void* stage2, float* means, void* out, int out_dtype,
                          float m0, float m1, float m2, float s0, float s1, float s2, hipStream_t st) {
    if (N <= 0 || N > 65535 || S <= 0 || fill < 0 || fill > 255 || mix_dev == nullptr || stage == nullptr || stage2 == nullptr ||
        stage2 == stage)
        return YOLO_ERR_ARG;
    return prep_run(src, table_dev, tiles_dev, affine_dev, mix_dev, N, S, fill, jitter, stage, stage2, means, out, out_dtype, m0, m1,
                    m2, s0, s1, s2, st);
}

// letterbox of N sources into the model's input in one launch: src as above, table_dev = N yolo_letter_fill records, out:
// [N][3][S][S] of out_dtype
int yolo_letterbox(const void* src, const void* table_dev, int N, int S, int fill, void* out, int out_dtype, float m0, float m1,
                   float m2, float s0, float s1, float s2, hipStream_t st) {
    if (N <= 0 || N > 65535 || S <= 0 || S > 65535 || fill < 0 || fill > 255 || table_dev == nullptr || out == nullptr)
        return YOLO_ERR_ARG;
    YOLO_DISPATCH_T(out_dtype, hipLaunchKernelGGL((k_letterbox<T>), dim3(ceil_div(S, 256), S, N), dim3(256), 0, st,
                                                  (const unsigned char*)src, (const LetterRec*)table_dev, S, fill, (T*)out, m0, m1,
                                                  m2, s0, s1, s2));
    return YOLO_LAUNCH_CHECK();
}

}  // extern "C"
