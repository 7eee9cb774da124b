// resize_plan.hpp - host-side planner of the fused "resize + centre crop + normalise" launch (pcv_resize_crop_u8): plain C++, no
// HIP headers, so that a stand-alone program can include it (tests/tools/resize_plan_check.cpp runs it under the sanitizers).
//
// The resize is PIL's antialiased bilinear `Image.resize` as torchvision's `Resize(size)` calls it on a PIL image - what the
// reference's published error rates were produced with. It is an integer algorithm: two separable passes, horizontal first,
// 22-bit fixed-point coefficients, the intermediate rounded to uint8. Only the coefficients need floating point; they are made
// here in IEEE double WITHOUT fused multiply-add (a contracted `(xx + 0.5) * scale - support` rounds once instead of twice and
// can move a window bound), so that the kernel's part is integers only and reproduces PIL bit for bit.
//
// One axis, `in` source samples -> `out` output samples:
//   scale = in / out; fs = max(scale, 1); support = fs; ksize = ceil(support) * 2 + 1
//   output xx: center = (xx + 0.5) * scale; xmin = max((int)(center - support + 0.5), 0);
//              n = min((int)(center + support + 0.5), in) - xmin;
//              w[x] = max(0, 1 - |(x + xmin - center + 0.5) * (1 / fs)|), x < n, divided by their sum when that is non-zero;
//              kk[x] = (int)(0.5 + w[x] * 2^22)
//   a pass:    out_px = clamp((2^21 + sum_x src_px[xmin + x] * kk[x]) >> 22, 0, 255) in int32
// An axis whose size does not change gets kk = [2^22, 0]: the pass is the identity, PIL's "skip it" needs no special case.
//
// The blob (relocatable: offsets only, except each frame's device pointer):
//   ResizeHeader | ResizeFrame[N] | per distinct frame size: horizontal table of the W crop columns, vertical table of the H crop rows
//   a table of `count` outputs with `ksize` taps: int32 xmin[count], int32 n[count], int32 kk[count * ksize]
#ifndef PCV_RESIZE_PLAN_HPP
#define PCV_RESIZE_PLAN_HPP

#include <stdint.h>
#include <stddef.h>
#include <string.h>
#include <math.h>
#include <vector>

namespace pcv_resize {

constexpr uint32_t kMagic = 0x315A5352u;        // "RSZ1"
constexpr int kPrecisionBits = 22;              // PIL's PRECISION_BITS for 8-bit images (32 - 8 - 2)
// The kernel keeps a band's horizontally resampled source rows in LDS as uint8: at most this many bytes per block (the 64 KB a
// block gets without opting in to more; two blocks still share a CU). A frame that does not fit at ONE output row is refused.
constexpr int kStageBytes = 64 * 1024;
constexpr int kStageTarget = 24 * 1024;         // bands grow while they stay under this (occupancy), up to kMaxBandRows
constexpr int kMaxBandRows = 16;
constexpr int kMaxSide = 1 << 24;               // frame sides and `size`: keeps every int32 index of the planner in range

struct ResizeHeader {
    uint32_t magic;
    int32_t N, C, H, W;
    int32_t items;              // blocks' work items: sum of the frames' bands
    int32_t stage_bytes;        // LDS bytes a block needs (largest band of the batch, 16-byte multiple)
    int32_t reserved;
    uint64_t bytes;             // of the whole blob
    uint64_t src_bytes;         // source bytes the bands' row windows cover (what a launch reads at least; diagnostics)
};
static_assert(sizeof(ResizeHeader) == 48, "blob header layout");

struct ResizeFrame {
    uint64_t src;               // device pointer of the frame [Hs, Ws, C] uint8
    int32_t Hs, Ws;
    int32_t oh, ow;             // resized size (torchvision's rule for an int size)
    int32_t top, left;          // crop origin in the resized frame
    int32_t row0, row1;         // source rows [row0, row1) the H crop rows read
    int32_t hk, vk;             // taps per output (ksize) of the horizontal / vertical table
    int32_t band, nbands;       // output rows per block, number of bands (the last one may be shorter)
    int32_t item0;              // first work item of this frame
    int32_t reserved;
    uint32_t htab, vtab;        // byte offsets of the tables from the start of the blob
};
static_assert(sizeof(ResizeFrame) == 72, "blob frame layout");

struct Axis {
    int ksize = 0;
    std::vector<int32_t> xmin, n, kk;       // kk: [count][ksize], zero past n
};

// torchvision's output size for an int `size`: the shorter side becomes `size`, the other int(size * long / short) (true division,
// truncation).
// Returns false when the long side would pass kMaxSide.
inline bool output_size(int h, int w, int size, int* oh, int* ow) {
    const double lng = w <= h ? (double)size * (double)h / (double)w : (double)size * (double)w / (double)h;
    if (lng > (double)kMaxSide) return false;
    if (w <= h) {
        *ow = size;
        *oh = (int)lng;
    } else {
        *oh = size;
        *ow = (int)lng;
    }
    return true;
}

// torchvision's CenterCrop origin: int(round((full - crop) / 2.0)) with Python's round-half-to-even.
inline int crop_origin(int full, int crop) {
    const int d = full - crop;
    return (d & 1) ? ((d / 2) & 1 ? d / 2 + 1 : d / 2) : d / 2;
}

// Coefficients of outputs [first, first + count) of an axis in -> out (see the head of this file); `weights` false: the windows
// (xmin, n) only, which is all that sizing and the refusals need.
#if defined(__GNUC__) && !defined(__clang__)
__attribute__((optimize("fp-contract=off")))
#endif
inline void axis_coeffs(int in, int out, int first, int count, Axis& a, bool weights = true) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double scale = (double)in / (double)out;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = fs;
    const double ss = 1.0 / fs;
    const int ksize = (int)ceil(support) * 2 + 1;
    a.ksize = ksize;
    a.xmin.assign(count, 0);
    a.n.assign(count, 0);
    a.kk.assign(weights ? (size_t)count * ksize : 0, 0);
    std::vector<double> w(weights ? ksize : 0);
    for (int i = 0; i < count; ++i) {
        const int xx = first + i;
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in) xmax = in;
        xmax -= xmin;
        a.xmin[i] = xmin;
        a.n[i] = xmax;
        if (!weights) continue;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) {
            double t = (x + xmin - center + 0.5) * ss;
            if (t < 0.0) t = -t;
            w[x] = t < 1.0 ? 1.0 - t : 0.0;
            ww += w[x];
        }
        for (int x = 0; x < xmax; ++x) {
            if (ww != 0.0) w[x] /= ww;
            a.kk[(size_t)i * ksize + x] = (int32_t)(0.5 + w[x] * (double)(1 << kPrecisionBits));
        }
    }
}

inline size_t table_bytes(int count, int ksize) { return ((size_t)count * 2 + (size_t)count * ksize) * sizeof(int32_t); }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// Everything about one frame but its tables' place in the blob.
struct FramePlan {
    ResizeFrame g;
    Axis h, v;
    int stage_bytes = 0;
    uint64_t src_bytes = 0;
};

// LDS bytes of the largest band when a block takes `band` output rows: (source rows of the band) x (W * C bytes, rounded to 4).
inline long long band_stage_bytes(const Axis& v, int H, int band, int pitch) {
    long long worst = 0;
    for (int y0 = 0; y0 < H; y0 += band) {
        const int y1 = y0 + band < H ? y0 + band : H;
        int lo = v.xmin[y0], hi = lo;
        for (int y = y0; y < y1; ++y) {
            if (v.xmin[y] < lo) lo = v.xmin[y];
            if (v.xmin[y] + v.n[y] > hi) hi = v.xmin[y] + v.n[y];
        }
        if ((long long)(hi - lo) * pitch > worst) worst = (long long)(hi - lo) * pitch;
    }
    return worst;
}

inline int stage_pitch(int W, int C) { return (W * C + 3) & ~3; }

// nullptr, or why the frame / the request is refused. `weights` false: geometry, band choice and table sizes only.
inline const char* plan_frame(int Hs, int Ws, int C, int size, int H, int W, FramePlan& p, bool weights = true) {
    if (C < 1 || C > 4) return "C must be 1..4";
    if (size <= 0 || H <= 0 || W <= 0 || size > kMaxSide) return "size, H and W must be positive";
    if (Hs <= 0 || Ws <= 0 || Hs > kMaxSide || Ws > kMaxSide) return "frame sides must be 1..2^24";
    int oh, ow;
    if (!output_size(Hs, Ws, size, &oh, &ow)) return "the resized frame is too large";
    if (oh < H || ow < W) return "the crop is larger than the resized frame";
    memset(&p.g, 0, sizeof(p.g));
    p.g.Hs = Hs; p.g.Ws = Ws; p.g.oh = oh; p.g.ow = ow;
    p.g.top = crop_origin(oh, H);
    p.g.left = crop_origin(ow, W);
    const int pitch = stage_pitch(W, C);
    // The taps per output grow with the scale, and both axes have (nearly) the same: an output row reads at least scale - 1 source
    // rows, so a scale this large is refused before tables are made that could not be used (which also bounds their size).
    static const char* const too_wide =
        "the source-row window of one output row does not fit the kernel's staging (the down-scale is too large)";
    if (((double)Hs / oh - 1.0) * pitch > kStageBytes || ((double)Ws / ow - 1.0) * pitch > kStageBytes) return too_wide;
    axis_coeffs(Ws, ow, p.g.left, weights ? W : 0, p.h, weights);
    axis_coeffs(Hs, oh, p.g.top, H, p.v, weights);
    p.g.hk = p.h.ksize;
    p.g.vk = p.v.ksize;
    int lo = p.v.xmin[0], hi = lo;
    for (int y = 0; y < H; ++y) {
        if (p.v.xmin[y] < lo) lo = p.v.xmin[y];
        if (p.v.xmin[y] + p.v.n[y] > hi) hi = p.v.xmin[y] + p.v.n[y];
    }
    p.g.row0 = lo;
    p.g.row1 = hi;
    if (band_stage_bytes(p.v, H, 1, pitch) > kStageBytes) return too_wide;
    int band = 1;
    for (int b = (H < kMaxBandRows ? H : kMaxBandRows); b > 1; --b)
        if (band_stage_bytes(p.v, H, b, pitch) <= kStageTarget) {
            band = b;
            break;
        }
    p.g.band = band;
    p.g.nbands = (H + band - 1) / band;
    p.stage_bytes = (int)align16((size_t)band_stage_bytes(p.v, H, band, pitch));
    p.src_bytes = 0;
    for (int y0 = 0; y0 < H; y0 += band) {
        const int yl = (y0 + band < H ? y0 + band : H) - 1;
        p.src_bytes += (uint64_t)(p.v.xmin[yl] + p.v.n[yl] - p.v.xmin[y0]) * Ws * C;
    }
    return nullptr;
}

inline const char* check_batch(int N, const int* hs, const int* ws) {
    if (N <= 0) return "N must be positive";
    if (!hs || !ws) return "NULL size array";
    return nullptr;
}

// Frames of one size share their tables (ImageNet's most common size is a quarter of it): the index of the first frame of the
// batch with frame i's size, i itself when there is none before it.
inline int first_of_size(const int* hs, const int* ws, int i, std::vector<int>& distinct) {
    for (int j : distinct)
        if (hs[j] == hs[i] && ws[j] == ws[i]) return j;
    distinct.push_back(i);
    return i;
}

// Size of the blob for a batch; nullptr or the refusal.
inline const char* plan_bytes(int N, const int* hs, const int* ws, int C, int size, int H, int W, size_t* bytes) {
    if (const char* why = check_batch(N, hs, ws)) return why;
    size_t total = align16(sizeof(ResizeHeader) + (size_t)N * sizeof(ResizeFrame));
    FramePlan p;
    std::vector<int> distinct;
    for (int i = 0; i < N; ++i) {
        if (first_of_size(hs, ws, i, distinct) != i) continue;
        if (const char* why = plan_frame(hs[i], ws[i], C, size, H, W, p, false)) return why;
        total += align16(table_bytes(W, p.h.ksize)) + align16(table_bytes(H, p.v.ksize));
        if (total >= 0x7fffffffu) return "the plan exceeds 2 GiB; split the batch";
    }
    *bytes = total;
    return nullptr;
}

inline void write_table(char* dst, const Axis& a) {
    const size_t count = a.xmin.size();
    memcpy(dst, a.xmin.data(), count * 4);
    memcpy(dst + count * 4, a.n.data(), count * 4);
    memcpy(dst + count * 8, a.kk.data(), a.kk.size() * 4);
}

// Fills `blob` (host memory, `bytes` long = plan_bytes' answer); frames[i] is the device pointer of frame i.
inline const char* plan(const void* const* frames, int N, const int* hs, const int* ws, int C, int size, int H, int W, void* blob,
                        size_t bytes) {
    if (!frames || !blob) return "NULL argument";
    size_t need = 0;
    if (const char* why = plan_bytes(N, hs, ws, C, size, H, W, &need)) return why;
    if (need != bytes) return "bytes is not what pcv_resize_plan_bytes gives for this batch";
    char* base = static_cast<char*>(blob);
    memset(base, 0, bytes);
    ResizeHeader hd;
    memset(&hd, 0, sizeof(hd));
    hd.magic = kMagic; hd.N = N; hd.C = C; hd.H = H; hd.W = W; hd.bytes = bytes;
    size_t off = align16(sizeof(ResizeHeader) + (size_t)N * sizeof(ResizeFrame));
    FramePlan p;
    long long items = 0;
    std::vector<int> distinct;
    std::vector<uint64_t> src_bytes(N);
    for (int i = 0; i < N; ++i) {
        if (!frames[i]) return "NULL frame pointer";
        char* rec = base + sizeof(ResizeHeader) + (size_t)i * sizeof(ResizeFrame);
        const int j = first_of_size(hs, ws, i, distinct);
        if (j != i) {                                       // same size as frame j: same geometry, same tables
            memcpy(&p.g, base + sizeof(ResizeHeader) + (size_t)j * sizeof(ResizeFrame), sizeof(p.g));
            src_bytes[i] = src_bytes[j];
        } else {
            if (const char* why = plan_frame(hs[i], ws[i], C, size, H, W, p)) return why;
            p.g.htab = (uint32_t)off;
            write_table(base + off, p.h);
            off += align16(table_bytes(W, p.h.ksize));
            p.g.vtab = (uint32_t)off;
            write_table(base + off, p.v);
            off += align16(table_bytes(H, p.v.ksize));
            if (p.stage_bytes > hd.stage_bytes) hd.stage_bytes = p.stage_bytes;
            src_bytes[i] = p.src_bytes;
        }
        p.g.src = (uint64_t)(uintptr_t)frames[i];
        p.g.item0 = (int32_t)items;
        items += p.g.nbands;
        if (items > 0x3fffffff) return "too many bands; split the batch";
        memcpy(rec, &p.g, sizeof(p.g));
        hd.src_bytes += src_bytes[i];
    }
    hd.items = (int32_t)items;
    memcpy(base, &hd, sizeof(hd));
    return off == bytes ? nullptr : "internal: blob size mismatch";
}

// What the launch re-checks on the HOST copy before it trusts the geometry: nullptr or the complaint.
inline const char* validate(const void* blob, size_t bytes) {
    if (!blob || bytes < sizeof(ResizeHeader)) return "plan too short";
    ResizeHeader hd;
    memcpy(&hd, blob, sizeof(hd));
    if (hd.magic != kMagic) return "not a resize plan (bad magic)";
    if (hd.bytes != bytes) return "bytes differs from the plan's own size";
    if (hd.N <= 0 || hd.C < 1 || hd.C > 4 || hd.H <= 0 || hd.W <= 0 || hd.items <= 0 || hd.stage_bytes <= 0 ||
        hd.stage_bytes > kStageBytes || sizeof(ResizeHeader) + (size_t)hd.N * sizeof(ResizeFrame) > bytes)
        return "corrupt plan header";
    const int pitch = stage_pitch(hd.W, hd.C);
    long long items = 0;
    for (int i = 0; i < hd.N; ++i) {
        ResizeFrame g;
        memcpy(&g, static_cast<const char*>(blob) + sizeof(ResizeHeader) + (size_t)i * sizeof(ResizeFrame), sizeof(g));
        if (!g.src || g.Hs <= 0 || g.Ws <= 0 || g.hk < 3 || g.vk < 3 || g.band < 1 || g.nbands != (hd.H + g.band - 1) / g.band ||
            g.item0 != items || g.row0 < 0 || g.row1 > g.Hs || g.row0 >= g.row1 ||
            (size_t)g.htab + table_bytes(hd.W, g.hk) > bytes || (size_t)g.vtab + table_bytes(hd.H, g.vk) > bytes || (g.htab & 15) ||
            (g.vtab & 15))
            return "corrupt plan frame";
        // the bands' row windows against the staging the launch will ask for
        const int32_t* vt = reinterpret_cast<const int32_t*>(static_cast<const char*>(blob) + g.vtab);
        for (int y0 = 0; y0 < hd.H; y0 += g.band) {
            const int yl = (y0 + g.band < hd.H ? y0 + g.band : hd.H) - 1;
            const long long r0 = vt[y0], r1 = (long long)vt[yl] + vt[hd.H + yl];
            if (r0 < 0 || r1 > g.Hs || r1 <= r0 || (r1 - r0) * pitch > hd.stage_bytes) return "corrupt plan band";
            for (int y = y0; y <= yl; ++y)
                if (vt[y] < r0 || vt[hd.H + y] < 1 || vt[hd.H + y] > g.vk || (long long)vt[y] + vt[hd.H + y] > r1)
                    return "corrupt plan rows";
        }
        const int32_t* ht = reinterpret_cast<const int32_t*>(static_cast<const char*>(blob) + g.htab);
        for (int x = 0; x < hd.W; ++x)
            if (ht[x] < 0 || ht[hd.W + x] < 1 || ht[hd.W + x] > g.hk || (long long)ht[x] + ht[hd.W + x] > g.Ws)
                return "corrupt plan columns";
        items += g.nbands;
    }
    if (items != hd.items) return "corrupt plan (band count)";
    return nullptr;
}

}  // namespace pcv_resize
#endif  // PCV_RESIZE_PLAN_HPP
