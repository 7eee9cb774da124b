// pcv_api.hip - host side of the C ABI declared in include/pcv_amd.h: argument checking, convolution planning
// (K-chunk tables, group blocking, tile choice) and kernel launches. No torch, no exceptions across the boundary.
#include <hip/hip_runtime.h>
#include <string>
#include <type_traits>
#include <vector>
#include <cstring>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <dlfcn.h>
#include "pcv_common.hpp"
#include "igemm_inst.hpp"
#include "d3q_inst.hpp"
#include "d3w_inst.hpp"
#include "d3c_conv.hpp"
#include "d3k_conv.hpp"
#include "d3i_conv.hpp"
#include "d1i_conv.hpp"
#include "p1r_conv.hpp"
#include "stem_conv.hpp"
#include "pair1x1.hpp"
#include "wpair1x1.hpp"
#include "bnu.hpp"
#include "gconv3x3.hpp"
#include "gconv3x3r.hpp"
#include "gconvx.hpp"
GCONVX_INSTANCES(GCONVX_DECLARE, PCV_BF16)
GCONVX_INSTANCES(GCONVX_DECLARE, PCV_F16)
#include "mbconv.hpp"
#include "mbw_inst.hpp"
#include "mbr_inst.hpp"
MBW_SHAPES(MBW_DECLARE, PCV_BF16)
MBW_SHAPES(MBW_DECLARE, PCV_F16)
MBW2_SHAPES(MBW2_DECLARE, PCV_BF16)
MBW2_SHAPES(MBW2_DECLARE, PCV_F16)
MBW3_SHAPES(MBW3_DECLARE, PCV_BF16)
MBW3_SHAPES(MBW3_DECLARE, PCV_F16)
MBR_SHAPES(MBR_DECLARE, PCV_BF16)
MBR_SHAPES(MBR_DECLARE, PCV_F16)
#include "dwconv.hpp"
#include "mixconv.hpp"
MIX_INSTANCES(MIX_DECLARE, PCV_F32)
MIX_INSTANCES(MIX_DECLARE, PCV_BF16)
MIX_INSTANCES(MIX_DECLARE, PCV_F16)
#include "ghost.hpp"
GHOST_INSTANCES(GHOST_DECLARE, PCV_F32)
GHOST_INSTANCES(GHOST_DECLARE, PCV_BF16)
GHOST_INSTANCES(GHOST_DECLARE, PCV_F16)
#include "aux_kernels.hpp"
#include "cbam_kernels.hpp"
#include "instnorm.hpp"
#include "hrfuse.hpp"
#include "resize_kernel.hpp"
#include "classify_kernel.hpp"
#include "head_gemm.hpp"


IGEMM_INSTANCES(IGEMM_DECLARE, PCV_BF16)
IGEMM_INSTANCES(IGEMM_DECLARE, PCV_F16)
IGEMM_INSTANCES_SAMETYPE(IGEMM_DECLARE, PCV_F32)
D3Q_SHAPES(D3Q_DECLARE, PCV_BF16)
D3Q_SHAPES(D3Q_DECLARE, PCV_F16)
D3Q1_SHAPES(D3Q1_DECLARE, PCV_BF16)
D3Q1_SHAPES(D3Q1_DECLARE, PCV_F16)
D3W_SHAPES(D3W_DECLARE, PCV_BF16)
D3W_SHAPES(D3W_DECLARE, PCV_F16)
D3WT_SHAPES(D3WT_DECLARE, PCV_BF16)
D3WT_SHAPES(D3WT_DECLARE, PCV_F16)
extern template __global__ void d3c_kernel<PCV_BF16>(const D3Params);
extern template __global__ void d3c_kernel<PCV_F16>(const D3Params);
extern template __global__ void d3k_kernel<PCV_BF16>(const D3Params);
extern template __global__ void d3k_kernel<PCV_F16>(const D3Params);
extern template __global__ void d3i_kernel<PCV_BF16, 256>(const D3Params);
extern template __global__ void d3i_kernel<PCV_F16, 256>(const D3Params);
extern template __global__ void d3i_kernel<PCV_BF16, 512>(const D3Params);
extern template __global__ void d3i_kernel<PCV_F16, 512>(const D3Params);
extern template __global__ void d1i_kernel<PCV_BF16, 1024>(const D3Params);
extern template __global__ void d1i_kernel<PCV_F16, 1024>(const D3Params);
extern template __global__ void d1i_kernel<PCV_BF16, 2048>(const D3Params);
extern template __global__ void d1i_kernel<PCV_F16, 2048>(const D3Params);
#define P1R_DECLARE(CW, CIN)                                                       \
    extern template __global__ void p1r_kernel<PCV_BF16, CW, CIN>(const D3Params); \
    extern template __global__ void p1r_kernel<PCV_F16, CW, CIN>(const D3Params);
P1R_DECLARE(64, 256)
P1R_DECLARE(32, 512)
P1R_DECLARE(32, 256)
#define BNU_DECLARE(DT)                                                          \
    extern template __global__ void bnu_kernel<DT, false>(const BnuParams);      \
    extern template __global__ void bnu_kernel<DT, true>(const BnuParams);
BNU_DECLARE(PCV_BF16)
BNU_DECLARE(PCV_F16)

enum TileCfg { TILE_C32 = 0, TILE_C64 = 1, TILE_C128 = 2, TILE_C256 = 3, TILE_C64S = 4, TILE_C128S = 5, TILE_COUNT = 6 };

struct pcv_ctx {
    int device = 0;
    std::string err;
    int num_cu = 256;
    int persist_mode = 1;       // 1 always (measured best on every ResNet-50 layer), 0 never, -1 by K-steps (PCV_AMD_PERSIST)
    int force_tile = -1;        // tuning only: force the implicit-GEMM tile (0..3) where legal
    int use_wstat = 1;          // weight-stationary persistent mode for single-K-step layers
    int use_mbr = 1;            // stride-1 fused inverted-residual units with Cin <= 32 run the register-resident kernel (mbr.hpp); 0: mbw.hpp / mbconv.hpp
    int use_mbr_xl = 1;         // mbr.hpp instantiations that stage x through LDS; 0: never (A/B)
    int use_mbw = 1;            // fused inverted-residual units with Cin <= 32 run the wave-private kernel (mbw.hpp; 8 / 16: force that pixel-block width); 0: mbconv.hpp
    int use_gconvr = 1;         // grouped 3x3 stride 2 / 32 channels per group on the row-tile kernel (gconv3x3r.hpp); 0 = generic implicit GEMM
    int use_gconvx = 1;         // grouped 3x3 at the group widths gconv3x3(r).hpp do not take (8..64 channels per group, any channel count) on gconvx.hpp; 0 (or "gconvr" 0) = generic implicit GEMM
    int use_d1x1 = -1;          // K-heavy 1x1 layers on d3q_kernel's 1x1 mode: -1 = pick_d1x1, 0 = never, n > 0 = force shape n - 1 where eligible
    int use_head = 1;           // fp32 dense layers on 1x1 maps run head_gemm.hpp (0: the generic implicit-GEMM tiles)
    int use_stem32 = 1;         // stems with <= 32 output channels run the 32-row form of the stem kernel (0: the 64-row form; A/B, tests)
    int use_d3x3 = -1;          // 8-wave dense 3x3 kernel (d3x3_conv.hpp): -1 = where eligible (16-bit, s1/p1, Cin % 64 == 0) with the tile shape
                                // the cost model picks, 0 = never, n > 0 = always with tile shape n - 1 (tests / sweeps)
    unsigned long long dbg_ptr = 0;   // diagnostic builds (-DD3X3_STAMPS): device buffer for in-kernel stamps ("dbg_lo" / "dbg_hi")
    int use_p1r = -1;           // 1x1 kernel with register-resident weights (p1r_conv.hpp; 256 / 512 input channels): -1 = where it applies and fills the chip, 0 = never, 1 = wherever it applies, 3 = the same without the split tail round (A/B)
    int use_d3k = -1;           // 128-input-channel dense 3x3 kernel on 28-wide maps (d3k_conv.hpp): -1 = where it applies and fills the chip, 0 = never, 1 = wherever it applies
    int use_d3i = -1;           // dense 3x3 kernel with the image(s) in LDS (d3i_conv.hpp; 256 input channels on maps up to 14 x 14, 512 up to 7 x 7): -1 = where it applies and fills 3/4 of the chip, 0 = never, 1 = wherever it applies
    int use_d1i = -1;           // 1x1 kernel for 1024 / 2048 input channels with streamed activations and weights straight from L2 (d1i_conv.hpp): -1 = where it applies and pays, 0 = never, 1 = wherever it applies
    int use_d3c = -1;           // 64-input-channel dense 3x3 kernel on 56-wide maps (d3c_conv.hpp): -1 = where it applies and fills the chip, 0 = never, 1 = wherever it applies, 3 = the same without the split tail round (A/B)
    int use_d3w = -1;           // large-tile dense 3x3 kernel (d3w_conv.hpp): -1 = pick_d3w, 0 = never, n > 0 = force shape n - 1
    int dbg_flags = 0;          // timing experiments only ("dbg"): handed to the kernels that read it (d3q_conv.hpp: D3Params::dbgflags)
    int dw_flags = 0;           // tuning: bit 0 = non-temporal stores in the depthwise kernels
    int dw_th = 0;              // tuning: rows per thread of the depthwise kernel (0 = automatic)
    int max_blocks = 0;         // test-only: cap on every persistent grid (0 = resident blocks), so that small fixtures walk several
                                // tiles per block through the cross-tile pipelines (pcv_set_tuning("max_blocks", n))
    int bnu_band = 0;           // fused stage-1 bottleneck unit (bnu.hpp): rows per band, 0 = whole images once they fill the chip, else bands of >= 4 rows (tests: any value)
    int pair_pb = 2;            // fused 1x1 pair: 16-pixel blocks per tile (2: two blocks per CU, 4: one 512-register block)
    int persist_max_nk = 4;     // auto: persistent when a tile has at most this many K-steps (PCV_AMD_PERSIST_NK)
    uint32_t* ovf = nullptr;    // device word: how many threads have rounded a value beyond fp16's range so far (F16Guard, pcv_common.hpp);
                                // monotonic, never reset - pcv_fp16_guard_begin / _end compare two readings of it in stream order
    // Resident blocks per CU of the persistent kernels ON THIS DEVICE (enable_kernels: the occupancy query, floor 1). These kernels use
    // < 80 SGPRs, where the query is exact (MI355X_MICROARCH.md). Where one slot serves both 16-bit types it holds the fp16 instance's figure.
    int igemm_bpc[3][2][TILE_COUNT][3] = {};     // [dt][variant: 0 regular, 1 ragged/f32-out][tile][khw slot]
    int gconv_bpc[3] = {2, 2, 2};                // [gconv_slot(W)]
    int gconvx_bpc[2] = {2, 2};                  // [tile of 4 / 7 pixel blocks]: the widest group's (64 channels, stride 1), used by every width
    int stem_bpc[2] = {1, 1};                    // [bf16, fp16]: the plain 64-row form's, used by every form
    int pair_bpc[2] = {1, 1};                    // [PB == 4, PB == 2]; the gated form launches with [1]
    int pair_idc_bpc = 1;
    int wpair_bpc[4] = {1, 1, 1, 1};             // [wpair_cfg]: the ungated form's, used by both
};

static thread_local std::string g_create_err;

static int fail(pcv_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg; else g_create_err = msg;
    return code;
}
#define HIP_TRY(ctx, expr)                                                                          \
    do {                                                                                            \
        hipError_t e__ = (expr);                                                                    \
        if (e__ != hipSuccess)                                                                      \
            return fail(ctx, PCV_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__));      \
    } while (0)

// Launches go to the context's device whatever the caller's current device is (restored on return).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int want) {
        if (hipGetDevice(&prev) == hipSuccess && prev != want) switched = hipSetDevice(want) == hipSuccess;
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

// Every entry point that takes a context: a NULL context is refused without a message (there is nowhere to leave one), and the launches
// go to the context's device for the rest of the function. Two statements, the second a declaration: only as the FIRST statement of a
// function body.
#define PCV_ENTER(ctx)                       \
    if (!(ctx)) return PCV_ERR_INVALID;      \
    DeviceGuard device_guard((ctx)->device)
// ... and its last line after `<<<>>>` launches, which report through the runtime's sticky error
static int launched(pcv_ctx* ctx) {
    HIP_TRY(ctx, hipGetLastError());
    return PCV_OK;
}

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
// the test cap of pcv_set_tuning("max_blocks") on a grid of `blocks`
static inline long long cap_blocks(const pcv_ctx* ctx, long long blocks) {
    return (ctx->max_blocks > 0 && blocks > ctx->max_blocks) ? ctx->max_blocks : blocks;
}
// resident block slots of a persistent launch (CUs x blocks per CU), or that cap
static inline long long block_slots(const pcv_ctx* ctx, int per_cu) { return cap_blocks(ctx, (long long)ctx->num_cu * per_cu); }
static inline int esize(int dt) { return dt == PCV_F32 ? 4 : 2; }
static inline bool dtype_ok(int dt) { return dt == PCV_F32 || dt == PCV_BF16 || dt == PCV_F16; }
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// the 2 GiB that one launch's buffer descriptors address
static inline bool in_window(unsigned long long bytes) { return bytes < 0x80000000ull; }
static int too_large(pcv_ctx* ctx, const char* fn, const char* what) {
    return fail(ctx, PCV_ERR_TOO_LARGE, std::string(fn) + ": " + what + " exceeds the 2 GiB window of one launch; split the batch");
}
static const char* const kTensorTooLarge = "tensor exceeds the 2 GiB window";
// Grid of a flat launch, one thread per item: ceil(total / per_block) blocks, refused where a 32-bit grid does not hold the count (or
// the 64-bit product that gave `total` has wrapped to a negative value)
static int flat_grid(pcv_ctx* ctx, const char* fn, long long total, unsigned* grid, int per_block = 256) {
    const long long blocks = (total + per_block - 1) / per_block;
    if (total < 0 || blocks > 0x7fffffffll) return too_large(ctx, fn, "the grid");
    *grid = (unsigned)blocks;
    return PCV_OK;
}
// Grid of a streaming kernel over `total` 16-byte chunks: one short-lived block per 256 chunks - fresh blocks read 6.2 TB/s where
// grid-stride loops of resident blocks read 4.4 (tests/tools/micro/copy_bw2.cpp) - and the cap, which exists only so that the multi-round
// tests can make each block walk several rounds (max_blocks)
static int stream_grid(pcv_ctx* ctx, const char* fn, long long total, unsigned* grid) {
    if (int rc = flat_grid(ctx, fn, total, grid)) return rc;
    *grid = (unsigned)cap_blocks(ctx, *grid);
    return PCV_OK;
}
// The storage type as a template argument: f(tag) is called with decltype(tag)::value == dt, so a launch site names its kernel family
// once (`kernel<DT_OF(T)><<<...>>>(...)` inside a generic lambda). The entry points have checked dtype_ok(dt) before.
template <int V> using dtype_tag = std::integral_constant<int, V>;
#define DT_OF(tag) decltype(tag)::value
template <class F> static void for_dtype(int dt, F&& f) {
    if (dt == PCV_BF16) f(dtype_tag<PCV_BF16>{});
    else if (dt == PCV_F16) f(dtype_tag<PCV_F16>{});
    else f(dtype_tag<PCV_F32>{});
}
// the kernels that exist for the two 16-bit types only
template <class F> static void for_dtype16(int dt, F&& f) {
    if (dt == PCV_BF16) f(dtype_tag<PCV_BF16>{});
    else f(dtype_tag<PCV_F16>{});
}
// input type x output type {the same, fp32}: f(in, out)
template <class F> static void for_dtype_out(int dt, int ot, F&& f) {
    for_dtype(dt, [&](auto T) {
        if (ot == PCV_F32) f(T, dtype_tag<PCV_F32>{});
        else f(T, T);
    });
}

// One launchable kernel: entry point, block size, dynamic LDS bytes (the limit enable_kernels raises and the size launch() passes come
// from this one field) and, where the family has tile shapes, output channels x pixels of a tile. Each family below has one table or
// function that yields it from the selection parameters; enable_kernels walks the same.
struct Kernel { const void* fn; int threads, lds, BM, BP; };
template <class F> static Kernel kernel_of(F* fn, int threads, int lds, int BM = 0, int BP = 0) {
    return Kernel{reinterpret_cast<const void*>(fn), threads, lds, BM, BP};
}
template <class Params> static int launch(pcv_ctx* ctx, const Kernel& k, unsigned grid, hipStream_t stream, Params& q) {
    void* args[] = {&q};
    HIP_TRY(ctx, hipLaunchKernel(k.fn, dim3(grid), dim3((unsigned)k.threads), args, (size_t)k.lds, stream));
    return PCV_OK;
}
// resident blocks of `k` per CU of the current device (these kernels use < 80 SGPRs, where the query is exact - MI355X_MICROARCH.md)
static int blocks_per_cu(pcv_ctx* ctx, const Kernel& k, int* nb) {
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(nb, k.fn, k.threads, k.lds));
    if (*nb < 1) *nb = 1;
    return PCV_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Convolution plan: everything that depends on the descriptor but not on the data pointers.
// ---------------------------------------------------------------------------------------------------------
struct ConvPlan {
    bool stem = false;        // dedicated stem kernel (stem_conv.hpp): blob = [kh][64][32] weights, no K-chunk table
    bool conv3 = false;       // dedicated 3x3/s1/p1 kernel: K ordered (filter row, 128-byte channel slice, filter column)
    int ES = 2, CE = 8;
    bool pair = false;        // stem scheme: x_cpitch == 4 at 16 bit, one chunk = two pixels x 4 channels
    int Ho = 0, Wo = 0;
    int ngb = 1;              // group-blocks (blockIdx.y)
    int Cg_in = 0, Cg_out = 0;
    int cin_blk = 0, cout_blk = 0;
    int nR = 1, nQ = 1;
    int dy[IGEMM_MAX_TAPS], dx[IGEMM_MAX_TAPS];
    int nchunks = 0, nk = 0, Kpad = 0;
    int wrows = 0;
    size_t ktab_bytes = 0, w_bytes = 0, total_bytes = 0;
    int gconv_kt = 5;         // K-steps per slab of that blob: 5 (tap pairs x 16 channels; 4/8/16 channels per group) or 9 (taps x 32 channels)
    bool gconv = false;       // grouped 3x3/p1, stride 1 or 2, 4/8/16/32 channels per group: a second blob for gconv3x3(r).hpp follows the generic
    bool d3i = false;         // dense 3x3/s1/p1, 16 bit, 256 / 512 input channels, Cout % 64 == 0: a fragment-ordered copy of the weights for d3i_conv.hpp
    bool d1i = false;         // 1x1/s1, 16 bit, 1024 / 2048 input channels, Cout % 64 == 0: the same fragment-ordered copy for d1i_conv.hpp
    size_t d3i_off = 0;       // follows the generic blob (whether a launch takes that kernel depends on the map size)
    bool gconvx = false;      // grouped 3x3/p1, stride 1 or 2, Cin == Cout, 8/16/24/40/48/56/64 channels per group and not `gconv`: a blob for gconvx.hpp
    size_t gconvx_off = 0;    // behind the generic one (the launch may still fall back: pitches, a residual, an odd map at stride 2)
    size_t gconv_off = 0;     // one (the choice between the two kernels depends on the map width, known only at launch)
    std::vector<uint32_t> ktab;   // built only when tables == true
    std::vector<uint32_t> ksrc;
};

// A descriptor built by a binding that mirrors another layout of pcv_conv_desc (a stale ctypes stub) is refused, not read.
static const char* const kStaleDesc = "pcv_conv_desc.struct_size does not match this library (stale binding: compare pcv_conv_desc_size() / PCV_ABI_VERSION)";
static inline bool desc_stale(const pcv_conv_desc& d) { return d.struct_size != (int32_t)sizeof(pcv_conv_desc); }

// gconvx.hpp's group widths (GCONVX_WIDTHS): index into the kernel table, -1 = not one of them
static inline int gconvx_width(int cg) {
    static const int kWidths[7] = {8, 16, 24, 40, 48, 56, 64};
    for (int i = 0; i < 7; ++i)
        if (kWidths[i] == cg) return i;
    return -1;
}

static const char* plan_conv(const pcv_conv_desc& d, ConvPlan& P, bool tables) {
    if (desc_stale(d)) return kStaleDesc;
    if (!dtype_ok(d.dtype) || !dtype_ok(d.out_dtype)) return "unknown dtype";
    if (d.out_dtype != d.dtype && d.out_dtype != PCV_F32) return "out_dtype must equal dtype or be fp32";
    if (d.Cin <= 0 || d.Cout <= 0 || d.kh <= 0 || d.kw <= 0 || d.groups <= 0) return "non-positive conv dimension";
    // ranges first: everything below is 32-bit arithmetic on these fields (UBSan-clean for any descriptor: tests/test_host_sanitizers.py)
    constexpr int kMaxChannels = 1 << 20, kMaxExtent = 1 << 24, kMaxGeom = 1 << 12;
    if (d.Cin > kMaxChannels || d.Cout > kMaxChannels || d.groups > kMaxChannels) return "channel count out of range (> 2^20)";
    if (d.N < 0 || d.H < 0 || d.W < 0 || d.N > kMaxExtent || d.H > kMaxExtent || d.W > kMaxExtent) return "N / H / W out of range (> 2^24)";
    if (d.stride_h > kMaxGeom || d.stride_w > kMaxGeom || d.dil_h > kMaxGeom || d.dil_w > kMaxGeom) return "stride / dilation out of range";
    if (d.pad_t < 0 || d.pad_l < 0 || d.pad_b < 0 || d.pad_r < 0 || d.pad_t > kMaxGeom || d.pad_l > kMaxGeom || d.pad_b > kMaxGeom ||
        d.pad_r > kMaxGeom)
        return "padding out of range";
    if (d.x_cpitch < 0 || d.x_cpitch > 8 * kMaxChannels || d.x_wpitch < 0 || d.x_wpitch > 2 * kMaxExtent || d.y_cpitch < 0 ||
        d.y_cpitch > 8 * kMaxChannels)
        return "pitch out of range";
    if (d.kh >= IGEMM_MAX_TAPS || d.kw >= IGEMM_MAX_TAPS) return "kernel size > 15 unsupported";
    if (d.stride_h <= 0 || d.stride_w <= 0 || d.dil_h <= 0 || d.dil_w <= 0) return "non-positive stride/dilation";
    if (d.Cin % d.groups || d.Cout % d.groups) return "channels not divisible by groups";
    P.ES = esize(d.dtype);
    P.CE = 16 / P.ES;
    P.Cg_in = d.Cin / d.groups;
    P.Cg_out = d.Cout / d.groups;
    const int cpitch = d.x_cpitch > 0 ? d.x_cpitch : d.Cin;
    if (cpitch < d.Cin) return "x_cpitch < Cin";
    P.pair = (d.groups == 1 && cpitch == 4 && P.ES == 2);
    if (!P.pair && cpitch % P.CE != 0) return "x_cpitch must be a multiple of 16 bytes (or 4 for a padded 16-bit stem)";

    // group blocking: gpb whole groups per block, block-diagonal dense weights
    int gpb = 1;
    if (d.groups > 1) {
        while (gpb < d.groups && ((gpb * P.Cg_out) % 8 != 0 || (gpb * P.Cg_in) % P.CE != 0 || gpb * P.Cg_out < 32)) ++gpb;
        while (gpb < d.groups && d.groups % gpb != 0) ++gpb;
        if (d.groups % gpb != 0 || (gpb * P.Cg_out) % 8 != 0 || (gpb * P.Cg_in) % P.CE != 0)
            return "unsupported group shape (channels per group block not 16-byte aligned)";
    }
    P.ngb = d.groups / gpb;
    P.cin_blk = gpb * P.Cg_in;
    P.cout_blk = gpb * P.Cg_out;
    if (d.groups == 1) P.cin_blk = d.Cin;
    P.wrows = round_up(P.cout_blk, 32);

    P.conv3 = d.groups == 1 && d.kh == 3 && d.kw == 3 && d.stride_h == 1 && d.stride_w == 1 && d.dil_h == 1 && d.dil_w == 1 &&
              d.pad_t == 1 && d.pad_l == 1 && d.pad_b == 1 && d.pad_r == 1 && d.Cin % (8 * P.CE) == 0 && cpitch == d.Cin &&
              (d.x_wpitch <= 0 || d.x_wpitch == d.W) && d.out_dtype == d.dtype && d.Cout % 8 == 0;

    P.stem = P.pair && d.stride_h == 2 && d.stride_w == 2 && d.dil_h == 1 && d.Cout <= 64 && d.Cout % 8 == 0 && d.kh <= 7 &&
             d.kw + (d.pad_l & 1) <= 8 && d.out_dtype == d.dtype;

    // taps
    if (P.pair) {
        if (d.stride_w % 2 != 0 || d.dil_w != 1) return "padded 4-channel stem needs even stride_w and dilation 1";
        const int wp = d.x_wpitch > 0 ? d.x_wpitch : d.W;
        if (wp % 2 != 0) return "padded 4-channel stem needs an even x_wpitch";
        const int dxs = -(d.pad_l & 1);
        P.nQ = (d.kw - dxs + 1) / 2;
        P.nR = d.kh;
        if (P.nQ >= IGEMM_MAX_TAPS) return "stem too wide";
        for (int r = 0; r < P.nR; ++r) P.dy[r] = r * d.dil_h;
        for (int q = 0; q < P.nQ; ++q) P.dx[q] = dxs + 2 * q;
        P.nchunks = P.nR * P.nQ;
    } else {
        P.nR = d.kh;
        P.nQ = d.kw;
        for (int r = 0; r < P.nR; ++r) P.dy[r] = r * d.dil_h;
        for (int q = 0; q < P.nQ; ++q) P.dx[q] = q * d.dil_w;
        const int cchunks = (P.cin_blk + P.CE - 1) / P.CE;
        if (d.groups == 1 && cchunks * P.CE > cpitch) return "x_cpitch too small for the channel chunks";
        P.nchunks = P.nR * P.nQ * cchunks;
    }
    for (int i = P.nR; i < IGEMM_MAX_TAPS; ++i) P.dy[i] = 0;
    for (int i = P.nQ; i < IGEMM_MAX_TAPS; ++i) P.dx[i] = 0;
    P.nk = (P.nchunks + 7) / 8;
    P.Kpad = P.nk * 8 * P.CE;
    P.ktab_bytes = (size_t)round_up(P.nk * 8 * 8, 256);
    P.w_bytes = (size_t)P.ngb * P.wrows * P.Kpad * P.ES;
    P.total_bytes = P.ktab_bytes + P.w_bytes;
    // grouped 3x3: a second blob in gconv3x3.hpp's layout behind the generic one (everything here is static; whether the launch
    // can take that kernel also depends on the map width)
    static const bool gconv_on = !(std::getenv("PCV_AMD_GCONV") && std::atoi(std::getenv("PCV_AMD_GCONV")) == 0);
    P.gconv = gconv_on && d.groups > 1 && d.kh == 3 && d.kw == 3 && d.stride_h == d.stride_w && (d.stride_h == 1 || d.stride_h == 2) &&
              d.dil_h == 1 && d.dil_w == 1 &&
              d.pad_t == 1 && d.pad_l == 1 && d.pad_b == 1 && d.pad_r == 1 && d.Cin == d.Cout && d.Cin % 64 == 0 && P.ES == 2 &&
              (P.Cg_in == 4 || P.Cg_in == 8 || P.Cg_in == 16 || P.Cg_in == 32) && d.out_dtype == d.dtype;
    if (P.gconv) {
        P.gconv_kt = P.Cg_in == 32 ? 9 : 5;
        P.gconv_off = (P.total_bytes + 15) / 16 * 16;
        P.total_bytes = P.gconv_off + (size_t)(d.Cin / 16) * P.gconv_kt * 16 * 32 * P.ES;
    }
    P.gconvx = !P.gconv && d.groups > 1 && d.kh == 3 && d.kw == 3 && d.stride_h == d.stride_w && (d.stride_h == 1 || d.stride_h == 2) &&
               d.dil_h == 1 && d.dil_w == 1 && d.pad_t == 1 && d.pad_l == 1 && d.pad_b == 1 && d.pad_r == 1 && d.Cin == d.Cout && P.ES == 2 &&
               gconvx_width(P.Cg_in) >= 0 && d.out_dtype == d.dtype;
    if (P.gconvx) {
        P.gconvx_off = (P.total_bytes + 15) / 16 * 16;
        P.total_bytes = P.gconvx_off + (size_t)gconvx_packed_elems(d.groups, P.Cg_in) * P.ES;
    }
    P.d3i = P.conv3 && P.ES == 2 && (d.Cin == 256 || d.Cin == 512) && d.Cout % D3ICfg::CW == 0 && d.out_dtype == d.dtype &&
            P.wrows >= d.Cout && P.Kpad == 9 * d.Cin;
    if (P.d3i) {
        P.d3i_off = (P.total_bytes + 15) / 16 * 16;
        P.total_bytes = P.d3i_off + (size_t)(d.Cout / D3ICfg::CW) * (d.Cin == 256 ? D3ICfgT<256>::WBYTES : D3ICfgT<512>::WBYTES);
    }
    P.d1i = !P.conv3 && !P.pair && !P.stem && P.ES == 2 && d.kh == 1 && d.kw == 1 && d.groups == 1 && d.stride_h == 1 && d.stride_w == 1 &&
            d.pad_t == 0 && d.pad_l == 0 && d.pad_b == 0 && d.pad_r == 0 && (d.Cin == 1024 || d.Cin == 2048) &&
            d.Cout % 64 == 0 && d.out_dtype == d.dtype && P.wrows >= d.Cout && P.Kpad == d.Cin && P.ngb == 1;
    if (P.d1i) {
        P.d3i_off = (P.total_bytes + 15) / 16 * 16;
        P.total_bytes = P.d3i_off + (size_t)(d.Cout / 64) * (size_t)(d.Cin / 32) * 4096;
    }
    if (P.w_bytes >= 0x80000000ull) return "packed weights exceed 2 GiB";

    if (P.stem) {
        P.ktab_bytes = 0;
        P.w_bytes = (size_t)d.kh * 64 * 32 * P.ES;
        P.total_bytes = P.w_bytes;
    }
    // (a dilated filter larger than the padded input has no output: C's division rounds a negative extent towards zero, which at
    // stride >= 2 would make one output row / column out of nothing)
    const int eh = d.H + d.pad_t + d.pad_b - d.dil_h * (d.kh - 1) - 1, ew = d.W + d.pad_l + d.pad_r - d.dil_w * (d.kw - 1) - 1;
    P.Ho = eh < 0 ? 0 : eh / d.stride_h + 1;
    P.Wo = ew < 0 ? 0 : ew / d.stride_w + 1;

    if (tables) {
        P.ktab.assign((size_t)P.nk * 8 * 2, 0);
        P.ksrc.assign((size_t)P.Kpad, 0xFFFFFFFFu);
        const int khkw = d.kh * d.kw;
        (void)khkw;
        int j = 0;
        auto put = [&](int c0, int r, int q, int dyv, int dxv) {
            P.ktab[2 * j] = (uint32_t)c0 | ((uint32_t)r << 16) | ((uint32_t)q << 20);
            P.ktab[2 * j + 1] = ((uint32_t)dyv & 0xFFFFu) | (((uint32_t)dxv & 0xFFFFu) << 16);
            ++j;
        };
        if (P.pair) {
            for (int r = 0; r < P.nR; ++r)
                for (int q = 0; q < P.nQ; ++q) {
                    for (int e = 0; e < 8; ++e) {
                        const int pix = e >> 2, c = e & 3;
                        const int tap = P.dx[q] + pix;
                        if (tap >= 0 && tap < d.kw && c < d.Cin)
                            P.ksrc[(size_t)j * 8 + e] = (uint32_t)c | ((uint32_t)(r * d.kw + tap) << 16);
                    }
                    put(0, r, q, P.dy[r], P.dx[q]);
                }
        } else if (P.conv3) {
            const int slices = d.Cin / (8 * P.CE);
            for (int r = 0; r < 3; ++r)
                for (int cs = 0; cs < slices; ++cs)
                    for (int q = 0; q < 3; ++q)
                        for (int cc = cs * 8; cc < cs * 8 + 8; ++cc) {
                            for (int e = 0; e < P.CE; ++e)
                                P.ksrc[(size_t)j * P.CE + e] = (uint32_t)(cc * P.CE + e) | ((uint32_t)(r * 3 + q) << 16);
                            put(cc * P.CE, r, q, P.dy[r], P.dx[q]);
                        }
        } else {
            const int cchunks = (P.cin_blk + P.CE - 1) / P.CE;
            for (int r = 0; r < P.nR; ++r)
                for (int q = 0; q < P.nQ; ++q)
                    for (int cc = 0; cc < cchunks; ++cc) {
                        for (int e = 0; e < P.CE; ++e) {
                            const int c = cc * P.CE + e;
                            if (c < P.cin_blk)
                                P.ksrc[(size_t)j * P.CE + e] = (uint32_t)c | ((uint32_t)(r * d.kw + q) << 16);
                        }
                        put(cc * P.CE, r, q, P.dy[r], P.dx[q]);
                    }
        }
        while (j < P.nk * 8) put(0, 15, 0, 0, 0);      // r = 15 is never valid: zero-filled chunk
    }
    return nullptr;
}

// ---------------------------------------------------------------------------------------------------------
// Kernel table
// ---------------------------------------------------------------------------------------------------------
struct TileInfo { int BM, BP, threads, lds; };
static const TileInfo kTiles[TILE_COUNT] = {
    {32, 256, 256, 2 * (32 + 256) * 128},
    {64, 256, 256, 2 * (64 + 256) * 128},
    {128, 128, 256, 2 * (128 + 128) * 128},
    {256, 64, 256, 2 * (256 + 64) * 128},
    {64, 128, 256, 2 * (64 + 128) * 128},      // 1x1 only
    {128, 64, 256, 2 * (128 + 64) * 128},      // 1x1 only
};
typedef void (*igemm_fn)(const IgemmParams);

template <int DT, int KHW> static igemm_fn igemm_for_tile(int tile) {
    switch (tile) {
        case TILE_C32: return igemm_conv_kernel<DT, DT, 2, 4, 1, 4, false, KHW>;
        case TILE_C64: return igemm_conv_kernel<DT, DT, 4, 4, 1, 4, false, KHW>;
        case TILE_C128: return igemm_conv_kernel<DT, DT, 4, 4, 2, 2, false, KHW>;
        case TILE_C256: return igemm_conv_kernel<DT, DT, 4, 4, 4, 1, false, KHW>;
        case TILE_C64S: if constexpr (KHW == 1) return igemm_conv_kernel<DT, DT, 4, 2, 1, 4, false, 1>; else return nullptr;
        case TILE_C128S: if constexpr (KHW == 1) return igemm_conv_kernel<DT, DT, 4, 2, 2, 2, false, 1>; else return nullptr;
        default: return nullptr;
    }
}
template <int DT> static igemm_fn igemm_for_taps(int tile, int khw) {
    if (khw == 1) return igemm_for_tile<DT, 1>(tile);
    if (khw == 9) return igemm_for_tile<DT, 9>(tile);
    return igemm_for_tile<DT, 0>(tile);
}
// Non-ragged kernels store in the activation dtype; the ragged / fp32-output variants exist only on the 128x128 tile
// (classifier logits, odd channel counts) with descriptor-driven taps.
static igemm_fn igemm_fn_for(int dt, int ot, bool ragged, int tile, int khw) {
    if (!ragged && ot == dt) {
        if (dt == PCV_BF16) return igemm_for_taps<PCV_BF16>(tile, khw);
        if (dt == PCV_F16) return igemm_for_taps<PCV_F16>(tile, khw);
        return igemm_for_taps<PCV_F32>(tile, khw);
    }
    if (tile != TILE_C128) return nullptr;
    if (ot == PCV_F32) {
        if (dt == PCV_BF16) return igemm_conv_kernel<PCV_BF16, PCV_F32, 4, 4, 2, 2, true, 0>;
        if (dt == PCV_F16) return igemm_conv_kernel<PCV_F16, PCV_F32, 4, 4, 2, 2, true, 0>;
        return igemm_conv_kernel<PCV_F32, PCV_F32, 4, 4, 2, 2, true, 0>;
    }
    if (dt == PCV_BF16) return igemm_conv_kernel<PCV_BF16, PCV_BF16, 4, 4, 2, 2, true, 0>;
    if (dt == PCV_F16) return igemm_conv_kernel<PCV_F16, PCV_F16, 4, 4, 2, 2, true, 0>;
    return nullptr;
}

static Kernel igemm_kernel(int dt, int ot, bool ragged, int tile, int khw) {     // .fn == nullptr: no such instantiation
    const TileInfo& T = kTiles[tile];
    return kernel_of(igemm_fn_for(dt, ot, ragged, tile, khw), T.threads, T.lds, T.BM, T.BP);
}
static inline int khw_slot(int khw) { return khw == 1 ? 1 : (khw == 9 ? 2 : 0); }      // pcv_ctx::igemm_bpc

// ---------------------------------------------------------------------------------------------------------
static inline int gconv_slot(int W) { return W + 1 <= 16 ? 0 : (W + 1 <= 32 ? 1 : 2); }     // row width of the instantiation: 16 / 32 / 64
static Kernel gconv_kernel(int dt, int slot) {
    const bool bf = dt == PCV_BF16;
    if (slot == 0) return kernel_of(bf ? gconv3x3_kernel<PCV_BF16, 16> : gconv3x3_kernel<PCV_F16, 16>, 256, GConvCfg<16>::LDS);
    if (slot == 1) return kernel_of(bf ? gconv3x3_kernel<PCV_BF16, 32> : gconv3x3_kernel<PCV_F16, 32>, 256, GConvCfg<32>::LDS);
    return kernel_of(bf ? gconv3x3_kernel<PCV_BF16, 64> : gconv3x3_kernel<PCV_F16, 64>, 256, GConvCfg<64>::LDS);
}
// ---- row-tile grouped kernel (gconv3x3r.hpp): R whole output rows per tile, R Wo <= 64, window rows a multiple of 32 ----------
static const int kGconvRMaxLds = 160 * 1024;
// `lds`: what the launch's row plan needs (2 x window rows x 128 bytes); the default is the limit every instantiation is enabled for
static Kernel gconvr_kernel(int dt, int stride, int kt, int lds = kGconvRMaxLds) {
    const bool bf = dt == PCV_BF16;
    if (stride == 2) {
        if (kt == 9) return kernel_of(bf ? gconv3x3r_kernel<PCV_BF16, 2, 9> : gconv3x3r_kernel<PCV_F16, 2, 9>, 256, lds);
        return kernel_of(bf ? gconv3x3r_kernel<PCV_BF16, 2, 5> : gconv3x3r_kernel<PCV_F16, 2, 5>, 256, lds);
    }
    return kernel_of(bf ? gconv3x3r_kernel<PCV_BF16, 1, 9> : gconv3x3r_kernel<PCV_F16, 1, 9>, 256, lds);   // stride 1, <= 16 channels per group: gconv3x3.hpp
}
struct GConvRPlan { int R, XH, xl, win; };
static bool plan_gconvr(int stride, int H, int W, int Ho, int Wo, GConvRPlan& g) {
    if (stride == 2 && ((H | W) & 1)) return false;                // the flat-row identity needs H = 2 Ho, the parity split W = 2 Wo
    if (Wo > 64 || Ho <= 0) return false;
    for (int R = 64 / Wo; R >= 1; --R) {
        const int win = stride == 2 ? (2 * R + 1) * W + 2 : (R + 2) * W + 2;
        const int XH = stride == 2 ? ((win + 1) / 2 + 7) / 8 * 8 : 0;
        const int rows = ((stride == 2 ? 2 * XH : win) + 31) / 32 * 32;
        const int lds = 2 * rows * 128;
        if (lds * 2 <= kGconvRMaxLds || (R == 1 && lds <= kGconvRMaxLds)) {  // two blocks per CU; a wide map may take a whole CU's LDS
            g.R = R; g.XH = XH; g.xl = rows / 32; g.win = win;
            return true;
        }
    }
    return false;
}
// ---- any-width grouped kernel (gconvx.hpp): [bf16, fp16][stride - 1][pixel blocks 4, 7][gconvx_width] ---------------------------
#define GCONVX_KROW(DT, S, PB)                                                                                               \
    {kernel_of(gconvx_kernel<DT, S, 8, PB>, 256, kGConvXMaxLds), kernel_of(gconvx_kernel<DT, S, 16, PB>, 256, kGConvXMaxLds),  \
     kernel_of(gconvx_kernel<DT, S, 24, PB>, 256, kGConvXMaxLds), kernel_of(gconvx_kernel<DT, S, 40, PB>, 256, kGConvXMaxLds), \
     kernel_of(gconvx_kernel<DT, S, 48, PB>, 256, kGConvXMaxLds), kernel_of(gconvx_kernel<DT, S, 56, PB>, 256, kGConvXMaxLds), \
     kernel_of(gconvx_kernel<DT, S, 64, PB>, 256, kGConvXMaxLds)}
#define GCONVX_KTYPE(DT) {{GCONVX_KROW(DT, 1, 4), GCONVX_KROW(DT, 1, 7)}, {GCONVX_KROW(DT, 2, 4), GCONVX_KROW(DT, 2, 7)}}
static const Kernel kGConvX[2][2][2][7] = {GCONVX_KTYPE(PCV_BF16), GCONVX_KTYPE(PCV_F16)};
// The tile of a launch: R whole output rows (R Wo <= 112 pixels: the 4- or the 7-block instantiation) x GB whole groups.
//   * R: the largest (R + 2) / R (stride 2: (2 R + 1) / 2 R) of the window's rows are halo, so as many rows as the pixel cap and LDS
//     allow - but not at the price of fewer than four (group, slab) units, one per wave;
//   * GB: up to 128 channels (more units only lengthen a block's serial run), as many as the window leaves room for, then evened
//     out over the channel blocks (19 groups at 16 per block: 10 + 9, not 16 + 3).
// Everything here follows from the descriptor alone (pcv_gconvx_supported).
struct GConvXPlan { int R, GB, pbi, win, pitch, lds; };
static bool plan_gconvx(int stride, int H, int W, int Ho, int Wo, int groups, int Cg, GConvXPlan& g) {
    if (stride == 2 && ((H | W) & 1)) return false;                // the flat-row identity needs H = 2 Ho; even W keeps column 2 wo + 1 inside
    if (W > 112 || Ho <= 0 || Wo <= 0) return false;
    const int cpg = Cg / 8, sl = (Cg + 15) / 16;
    const int min_gb = std::min(groups, (4 + sl - 1) / sl);        // four units
    const int want_gb = std::min(groups, std::max(min_gb, 128 / Cg));
    for (int R = 16 * kGConvXPB[1] / Wo; R >= 1; --R) {
        const int win = stride == 2 ? (2 * R + 1) * W + 2 : (R + 2) * W + 2;
        int p16 = kGConvXMaxLds / (16 * win);                      // 16-byte chunks per window pixel that fit ...
        if (p16 % 2 == 0) --p16;                                   // ... as an odd pitch
        const int fit_gb = p16 / cpg;
        if (fit_gb < (R == 1 ? 1 : min_gb)) continue;
        int gb = std::min(want_gb, fit_gb);
        const int ncb = (groups + gb - 1) / gb;
        gb = (groups + ncb - 1) / ncb;
        g.R = R; g.GB = gb; g.pbi = R * Wo <= 16 * kGConvXPB[0] ? 0 : 1; g.win = win;
        g.pitch = 16 * ((gb * cpg) | 1);
        g.lds = win * g.pitch;
        return true;
    }
    return false;
}
// ---- 8-wave dense 3x3 kernel (d3q_conv.hpp) -----------------------------------------------------------------------------
// The kernels that share D3Params (launch_d3): one row per tile shape, [0] bf16, [1] fp16
template <class Cfg, class F> static Kernel tile_kernel(F* fn, int threads) { return kernel_of(fn, threads, Cfg::LDS, Cfg::BM, Cfg::BP); }
#define D3Q_ROW(DT, WC, WP, CBW, PBW, KS)                                                                   \
    {tile_kernel<D3Cfg<WC, WP, CBW, PBW, KS>>(d3q_kernel<PCV_BF16, WC, WP, CBW, PBW, KS>, 768),             \
     tile_kernel<D3Cfg<WC, WP, CBW, PBW, KS>>(d3q_kernel<PCV_F16, WC, WP, CBW, PBW, KS>, 768)},
static const Kernel kD3[][2] = {D3Q_SHAPES(D3Q_ROW, 0)};
static const int kD3Count = (int)(sizeof(kD3) / sizeof(kD3[0]));
// the same kernel in its 1x1 mode (K-heavy pointwise layers)
#define D3Q1_ROW(DT, WC, WP, CBW, PBW, KS)                                                                  \
    {tile_kernel<D3Cfg<WC, WP, CBW, PBW, KS, true>>(d3q_kernel<PCV_BF16, WC, WP, CBW, PBW, KS, true>, 768), \
     tile_kernel<D3Cfg<WC, WP, CBW, PBW, KS, true>>(d3q_kernel<PCV_F16, WC, WP, CBW, PBW, KS, true>, 768)},
static const Kernel kD1[][2] = {D3Q1_SHAPES(D3Q1_ROW, 0)};
static const int kD1Count = (int)(sizeof(kD1) / sizeof(kD1[0]));
// the large-tile kernel (d3w_conv.hpp): eight self-loading waves, 512 threads
#define D3W_ROW(DT, WC, WP, CBW, PBW, KS, NSA)                                                              \
    {tile_kernel<D3WCfg<WC, WP, CBW, PBW, KS, NSA>>(d3w_kernel<PCV_BF16, WC, WP, CBW, PBW, KS, NSA>, 512),  \
     tile_kernel<D3WCfg<WC, WP, CBW, PBW, KS, NSA>>(d3w_kernel<PCV_F16, WC, WP, CBW, PBW, KS, NSA>, 512)},
#define D3WT_ROW(DT, WC, WP, CBW, PBW, KS, NSA, TRIM)                                                                   \
    {tile_kernel<D3WCfg<WC, WP, CBW, PBW, KS, NSA, TRIM>>(d3w_kernel<PCV_BF16, WC, WP, CBW, PBW, KS, NSA, TRIM>, 512),  \
     tile_kernel<D3WCfg<WC, WP, CBW, PBW, KS, NSA, TRIM>>(d3w_kernel<PCV_F16, WC, WP, CBW, PBW, KS, NSA, TRIM>, 512)},
static const Kernel kD3W[][2] = {D3W_SHAPES(D3W_ROW, 0) D3WT_SHAPES(D3WT_ROW, 0)};
static const int kD3WCount = (int)(sizeof(kD3W) / sizeof(kD3W[0]));
// the register-weight kernels of ResNet stages 1 / 2 (256 threads, tiles = ROWS output rows of one image)
static const Kernel kD3C[1][2] = {{tile_kernel<D3CCfg>(d3c_kernel<PCV_BF16>, 256), tile_kernel<D3CCfg>(d3c_kernel<PCV_F16>, 256)}};
static const Kernel kD3K[1][2] = {{tile_kernel<D3KCfg>(d3k_kernel<PCV_BF16>, 256), tile_kernel<D3KCfg>(d3k_kernel<PCV_F16>, 256)}};
// d3i_conv.hpp: [0] 256, [1] 512 input channels; one block per (image(s), 256-channel tile), no pixel tiling
#define D3I_ROW(CIN)                                                                              \
    {kernel_of(d3i_kernel<PCV_BF16, CIN>, D3ICfg::THREADS, D3ICfgT<CIN>::LDS, D3ICfg::BM),        \
     kernel_of(d3i_kernel<PCV_F16, CIN>, D3ICfg::THREADS, D3ICfgT<CIN>::LDS, D3ICfg::BM)}
static const Kernel kD3I[2][2] = {D3I_ROW(256), D3I_ROW(512)};
// d1i_conv.hpp: [0] 1024, [1] 2048 input channels; the tile (256 channels x 208 pixels) and the LDS ring are those of the 1024 form for both
static const Kernel kD1I[2][2] = {
    {tile_kernel<D1ICfgT<1024>>(d1i_kernel<PCV_BF16, 1024>, 256), tile_kernel<D1ICfgT<1024>>(d1i_kernel<PCV_F16, 1024>, 256)},
    {tile_kernel<D1ICfgT<1024>>(d1i_kernel<PCV_BF16, 2048>, 256), tile_kernel<D1ICfgT<1024>>(d1i_kernel<PCV_F16, 2048>, 256)}};
// p1r_conv.hpp: [0] 256 input channels (8 waves x 64 channels), [1] 512 input channels (8 waves x 32 channels), [2] 256 input channels with
// 32 channels per wave (a skip tensor, or fewer than 384 output channels)
#define P1R_ROW(CW, CIN) \
    {tile_kernel<P1RCfg<CW, CIN>>(p1r_kernel<PCV_BF16, CW, CIN>, 512), tile_kernel<P1RCfg<CW, CIN>>(p1r_kernel<PCV_F16, CW, CIN>, 512)}
static const Kernel kP1R[3][2] = {P1R_ROW(64, 256), P1R_ROW(32, 512), P1R_ROW(32, 256)};
static const struct { const Kernel (*rows)[2]; int n; } kD3Tables[] = {{kD3, kD3Count}, {kD1, kD1Count}, {kD3W, kD3WCount}, {kD3C, 1},
                                                                       {kD3K, 1},       {kD3I, 2},       {kD1I, 2},         {kP1R, 3}};
// 1x1 mode: which pointwise layers go to the 8 + 4-wave kernel: K >= 256 and >= 128 output channels (the short-K layers keep the
// 4-wave kernel; where a fused pair applies the caller takes that first). Measured at batch 256 (us, generic -> this kernel):
// 512->256 @28x28 106 -> 90, 512->1024 + skip @14x14 93 -> 85, 256->1024 + skip 69 -> 60, 1024->512 74 -> 72, 2048->512 @7x7 43 -> 39;
// the 256 x 112 tile is 1-3 % ahead of 128 x 224 wherever the channel count fills it.
static int pick_d1x1(long long M, int Cout, int Cin, long long slots) {
    if (Cin < 256 || Cout < 128) return -1;
    const int shape = Cout % 256 == 0 ? 1 : 0;
    const long long tiles = (long long)((Cout + kD1[shape][0].BM - 1) / kD1[shape][0].BM) * ((M + kD1[shape][0].BP - 1) / kD1[shape][0].BP);
    return tiles * 2 >= slots ? shape : -1;                      // too few tiles to fill the chip with one block per CU: 4-wave kernel
}
// Tile shape for M pixels x Cout channels on `slots` CUs (one block each). With the activation tile staged once per filter row
// the bytes a K-step pulls through L2 are BM x 128 (weights) + BP x 128 / 3 (activations): wide pixel tiles with no more channel
// rows than needed. Measured on ResNet-50's four 3x3 layers (batch 256, us, generic -> this kernel): 64 ch 95 -> 85 (64 x 448),
// 128 ch 80 -> 69 (128 x 224), 256 ch 78 -> 64 (128 x 224; 256 x 112: 65), 512 ch 78 -> 63. The 64-pixel-per-wave shapes take over
// when the wide tile would leave more than half of the CUs without a tile; below a quarter of the CUs the generic 4-wave
// kernel (two blocks per CU, 128 x 128 tiles) fills the chip better: -1.
static int pick_d3x3(long long M, int Cout, int nk, long long slots) {
    (void)nk;
    const int wide = Cout <= 64 ? 2 : 1, narrow = Cout <= 64 ? 5 : 4;          // d3q_inst.hpp order
    auto tiles = [&](int i) { return ((Cout + kD3[i][0].BM - 1) / kD3[i][0].BM) * ((M + kD3[i][0].BP - 1) / kD3[i][0].BP); };
    // (512 channels at 7x7, batch 256: 224 tiles either way - 256 x 112 measured 66.9 / 70.9 us (plain / + skip) against 68.5 / 72.2 for 128 x 224)
    if (Cout % 256 == 0 && tiles(0) * 2 >= slots) return 0;
    if (tiles(wide) * 2 >= slots) return wide;
    if (tiles(narrow) * 4 >= slots) return narrow;
    return -1;
}
// Large-tile kernel (d3w_inst.hpp order: 0 / 1 = 256 x 224, 2 = 128 x 448, 3 = 64 x 448): layers whose output channels fill 256- or
// 128-row tiles and whose tile count fills at least three quarters of one round of CUs; -1 = leave the layer to d3q_kernel / the generic
// kernel. Measured at batch 256 (us, d3q -> this kernel): 256 ch @14x14 64.7 -> 55.3 (whole K-steps per interval; K-half intervals 57.1),
// 128 ch @28x28 70.4 -> 64.1; 64 ch @56x56 83.4 -> 84.9 and 512 ch @7x7 67.5 -> 73.5 (224 tiles of 128 x 224) stay on d3q.
static int pick_d3w(long long M, int Cout, long long slots) {
    const int shape = Cout % 256 == 0 ? 1 : (Cout % 128 == 0 ? 2 : -1);
    if (shape < 0) return -1;
    const long long tiles = (long long)(Cout / kD3W[shape][0].BM) * ((M + kD3W[shape][0].BP - 1) / kD3W[shape][0].BP);
    return tiles * 4 >= slots * 3 ? shape : -1;
}

// ---- stem kernel ------------------------------------------------------------------------------------------------------
static const int kStemLds = 7 * 64 * 64 + 2 * 768 * 16 + 3 * 2 * 64 * 16;     // weights + 2 patches + the pooled variant's row hand-down
enum StemForm { STEM_PLAIN = 0, STEM_POOLED = 1, STEM_NARROW = 2 };      // 64 channel rows; + fused max-pool; 32 channel rows (no pool)
// [bf16, fp16][x: padded NHWC4, fp32 NCHW (staged through kStemStageBytes more LDS)][StemForm]
#define STEM_ROWS(DT)                                                                                                          \
    {{kernel_of(stem_conv_kernel<DT, false>, 256, kStemLds), kernel_of(stem_conv_kernel<DT, true>, 256, kStemLds),             \
      kernel_of(stem_conv_kernel<DT, false, false, 2>, 256, kStemLds)},                                                        \
     {kernel_of(stem_conv_kernel<DT, false, true>, 256, kStemLds + kStemStageBytes),                                           \
      kernel_of(stem_conv_kernel<DT, true, true>, 256, kStemLds + kStemStageBytes),                                            \
      kernel_of(stem_conv_kernel<DT, false, true, 2>, 256, kStemLds + kStemStageBytes)}}
static const Kernel kStem[2][2][3] = {STEM_ROWS(PCV_BF16), STEM_ROWS(PCV_F16)};

static int pair_lds(int pb, bool idc = false) { return (idc ? 6 : 3) * 16 * pb * 64 * 2 + 16 * 1024 * pb + (idc ? 4096 : 0); }   // x (+ x0) ring + reduction buffer
enum PairForm { PAIR_PB4 = 0, PAIR_PB2 = 1, PAIR_GATED = 2, PAIR_IDCONV = 3 };     // (gated and identity-convolution forms: PB == 2)
#define PAIR_ROW(DT)                                                                                                          \
    {kernel_of(pair1x1_kernel<DT, 4>, 256, pair_lds(4)), kernel_of(pair1x1_kernel<DT, 2>, 256, pair_lds(2)),                  \
     kernel_of(pair1x1_kernel<DT, 2, false, true>, 256, pair_lds(2)), kernel_of(pair1x1_kernel<DT, 2, true>, 256, pair_lds(2, true))}
static const Kernel kPair[2][4] = {PAIR_ROW(PCV_BF16), PAIR_ROW(PCV_F16)};      // [bf16, fp16][PairForm]
// fused stage-1 bottleneck unit (bnu.hpp): [bf16, fp16][plain, identity-convolution form]; one 8-wave block per CU
#define BNU_ROW(DT) {kernel_of(bnu_kernel<DT, false>, 512, BnuCfg<false>::LDS), kernel_of(bnu_kernel<DT, true>, 512, BnuCfg<true>::LDS)}
static const Kernel kBnu[2][2] = {BNU_ROW(PCV_BF16), BNU_ROW(PCV_F16)};
static int g_bnu = -1;                  // "bnu": -1 = the fused unit where supported, 0 = never (process-wide: read by pcv_bottleneck_supported, which has no context)
// The two switches that stay process-wide: the context-free *_supported predicates of the ABI read them (pcv_set_tuning writes them
// through any context, for every context).
static int g_wpair_mask = 3;            // "wpair": bit 0: CM = 128, bit 1: CM = 256
static int g_mbw_wide = 1;              // "mbw_wide": mbw.hpp's units with 65..96 projected channels (mbw_shape)
// wide pair configurations: 0: 128 -> 512, 1: 256 -> 1024 (ResNet), 2: 128 -> 256, 3: 256 -> 512 (ResNeXt 32x4d)
struct WPairLaunch { Kernel k; int tileP; bool gate_in_lds; };
template <int CM, int C1> static WPairLaunch wpair_launch_for(int dt, bool gated) {
    typedef WPairCfg<CM, C1> G;
    const bool bf = dt == PCV_BF16;
    const int lds = gated ? G::LDS_GATED : G::LDS;
    const Kernel k = gated ? kernel_of(bf ? wpair1x1_kernel<PCV_BF16, CM, C1, true> : wpair1x1_kernel<PCV_F16, CM, C1, true>, 64 * G::NW, lds)
                           : kernel_of(bf ? wpair1x1_kernel<PCV_BF16, CM, C1, false> : wpair1x1_kernel<PCV_F16, CM, C1, false>, 64 * G::NW, lds);
    return WPairLaunch{k, G::P, gated && G::GATE_LDS};
}
static WPairLaunch wpair_launch(int cfg, int dt, bool gated = false) {
    switch (cfg) {
        case 0: return wpair_launch_for<128, 512>(dt, gated);
        case 1: return wpair_launch_for<256, 1024>(dt, gated);
        case 2: return wpair_launch_for<128, 256>(dt, gated);
        default: return wpair_launch_for<256, 512>(dt, gated);
    }
}
static int wpair_cfg(int cm, int c1) {
    if (cm == 128 && c1 == 512) return 0;
    if (cm == 256 && c1 == 1024) return 1;
    if (cm == 128 && c1 == 256) return 2;
    if (cm == 256 && c1 == 512) return 3;
    return -1;
}
// a 1x1 convolution with nothing but channels: stride 1, no padding, one group, dense x and y in the input's type
static bool plain_1x1(const pcv_conv_desc& d) {
    return d.kh == 1 && d.kw == 1 && d.stride_h == 1 && d.stride_w == 1 && d.pad_t == 0 && d.pad_l == 0 && d.pad_b == 0 &&
           d.pad_r == 0 && d.groups == 1 && d.dil_h == 1 && d.dil_w == 1 && d.out_dtype == d.dtype &&
           (d.x_cpitch == 0 || d.x_cpitch == d.Cin) && (d.x_wpitch == 0 || d.x_wpitch == d.W) &&
           (d.y_cpitch == 0 || d.y_cpitch == d.Cout);
}
// Which (conv, next conv) pairs the fused kernel covers: 1x1/s1 64 -> 256 with residual, then 1x1/s1 256 -> 64, 16 bit.
static const char* pair_unsupported(const pcv_conv_desc& a, const pcv_conv_desc& b) {
    if (desc_stale(a) || desc_stale(b)) return kStaleDesc;
    if (!plain_1x1(a) || !plain_1x1(b)) return "both convolutions must be plain 1x1 stride 1";
    if (a.dtype != b.dtype || (a.dtype != PCV_BF16 && a.dtype != PCV_F16)) return "16-bit storage only";
    if (a.N != b.N || a.H != b.H || a.W != b.W || a.Cout != b.Cin) return "shapes do not chain";
    const bool narrow = a.Cin == 64 && a.Cout == 256 && b.Cout == 64;        // pair1x1.hpp: weights in registers
    const bool wide = ((a.Cin == 128 && (g_wpair_mask & 1)) || (a.Cin == 256 && (g_wpair_mask & 2))) &&
                      wpair_cfg(a.Cin, a.Cout) >= 0 && b.Cout == a.Cin;   // wpair1x1.hpp: weights through an LDS ring
    if (!narrow && !wide) return "only 64 -> 256 -> 64, 128 -> 512|256 -> 128 and 256 -> 1024|512 -> 256 are instantiated";
    if (!a.has_residual || b.has_residual || b.post_act != PCV_ACT_NONE) return "first conv must carry the residual, second must not";
    if ((long)a.N * a.H * a.W * a.Cout * 2 >= (1L << 31)) return kTensorTooLarge;
    return nullptr;
}

// ---- fused inverted-residual unit (mbconv.hpp) ----------------------------------------------------------------------------
typedef void (*mbconv_fn)(const MbParams);
template <int DT> static mbconv_fn mbconv_for(int stride, bool expand) {
    if (stride == 1) return expand ? mbconv_kernel<DT, 1, true> : mbconv_kernel<DT, 1, false>;
    return expand ? mbconv_kernel<DT, 2, true> : mbconv_kernel<DT, 2, false>;
}
// The three fused-unit kernels size their LDS per unit (mbconv_plan / mbw_lds_layout / mbr_entry_lds): the launch passes that size as
// `lds`, the default is the limit every instantiation is enabled for.
static const int kMbMaxLds = 150 * 1024, kMbwMaxLds = 160 * 1024;
// block tiles (mbconv.hpp): compiled for kMbRowT = 2 projection row tiles, i.e. Cout <= 32
static Kernel mbconv_kernel(int dt, int stride, bool expand, int lds = kMbMaxLds) {
    return kernel_of(dt == PCV_BF16 ? mbconv_for<PCV_BF16>(stride, expand) : mbconv_for<PCV_F16>(stride, expand), 256, lds);
}
// wave-private variant (mbw.hpp): Cin <= 32, Cout <= 64
struct MbwEntry { int dt, s, nrt, act, tw, ka, rb; mbconv_fn fn; };
#define MBW_ROW(DT, S, NRT, ACT, TW) {DT, S, NRT, ACT, TW, 1, 0, mbw_kernel<DT, S, NRT, ACT, TW>},
#define MBW2_ROW(DT, S, NRT, ACT, TW, KA) {DT, S, NRT, ACT, TW, KA, 0, mbw_kernel<DT, S, NRT, ACT, TW, KA>},
#define MBW3_ROW(DT, S, NRT, ACT, TW, KA, RB) {DT, S, NRT, ACT, TW, KA, RB, mbw_kernel<DT, S, NRT, ACT, TW, KA, RB>},
static const MbwEntry kMbw[] = {MBW_SHAPES(MBW_ROW, PCV_BF16) MBW_SHAPES(MBW_ROW, PCV_F16) MBW2_SHAPES(MBW2_ROW, PCV_BF16)
                                MBW2_SHAPES(MBW2_ROW, PCV_F16) MBW3_SHAPES(MBW3_ROW, PCV_BF16) MBW3_SHAPES(MBW3_ROW, PCV_F16)};
// act: PCV_ACT_RELU / PCV_ACT_RELU6 when both inner activations are that one, anything else = the launch-time codes
static const MbwEntry* pick_mbw(int dt, int stride, int nrt, int act, int tw, int ka, int rb) {
    if (act != PCV_ACT_RELU && act != PCV_ACT_RELU6) act = -1;
    for (const MbwEntry& e : kMbw)
        if (e.dt == dt && e.s == stride && e.nrt == nrt && e.act == act && e.tw == tw && e.ka == ka && e.rb == rb) return &e;
    return nullptr;
}
static Kernel mbw_kernel_of(const MbwEntry& e, int waves = 8, int lds = kMbwMaxLds) { return kernel_of(e.fn, 64 * waves, lds); }
// register-resident variant (mbr.hpp): stride 1, Cin <= 32, Cout <= 64
struct MbrEntry { int dt, nrt, act, ro, s, ka; bool afl; int waves; bool wel, xl; mbconv_fn fn; };
#define MBR_ROW(DT, NRT, ACT, RO, S, KA, AFL, WV, WEL, XL) {DT, NRT, ACT, RO, S, KA, AFL, WV, WEL, XL, mbr_kernel<DT, NRT, ACT, RO, S, KA, AFL, WV, WEL, XL>},
static int mbr_entry_lds(const MbrEntry& e, int nChunks) {
    const int nr = e.s == 1 ? e.ro + 2 : 2 * e.ro + 1;
    return mbr_lds_layout(e.nrt, nChunks, e.ka, e.afl, e.wel, e.xl ? nr : 0, e.waves).total;
}
static const MbrEntry kMbr[] = {MBR_SHAPES(MBR_ROW, PCV_BF16) MBR_SHAPES(MBR_ROW, PCV_F16)};
static Kernel mbr_kernel_of(const MbrEntry& e, int lds = kMbwMaxLds) { return kernel_of(e.fn, 64 * e.waves, lds); }
// the instantiation for a unit, when its tables fit the LDS
static const MbrEntry* pick_mbr(const pcv_ctx* ctx, int dt, int nrt, int act, int stride, int ka, int nChunks) {
    if (act != PCV_ACT_RELU && act != PCV_ACT_RELU6) return nullptr;          // launch-time activations: mbw.hpp / mbconv.hpp (mbr_inst.hpp)
    for (const MbrEntry& e : kMbr)
        if (e.dt == dt && e.nrt == nrt && e.act == act && e.s == stride && e.ka == ka &&
            mbr_entry_lds(e, nChunks) <= kMbwMaxLds && (!e.xl || ctx->use_mbr_xl))
            return &e;
    return nullptr;
}
// waves per block (one block per CU): as many of 8 / 6 / 4 as the LDS holds beside the unit's weights; 0 = does not fit
static int mbw_waves(int stride, int nrt, int nChunks, int tw, int ka, int rb) {
    for (int nw = 8; nw >= 4; nw -= 2)
        if (mbw_lds_layout(stride, nrt, nChunks, nw, tw, ka, rb).total <= kMbwMaxLds) return nw;
    return 0;
}
// LDS plan of one unit: prefetch the next tile's x (two buffers) when that still leaves room for two blocks per CU
static MbLds mbconv_plan(int stride, bool expand, int ka, int nChunks, int nRowT, int* nbufX) {
    MbLds two = mb_lds_layout(stride, expand, ka, nChunks, nRowT, 2);
    if (!expand || two.total <= 80 * 1024) { *nbufX = 2; return two; }
    MbLds one = mb_lds_layout(stride, expand, ka, nChunks, nRowT, 1);
    if (one.total <= 80 * 1024 || two.total > kMbMaxLds) { *nbufX = 1; return one; }
    *nbufX = 2;
    return two;
}

// index of a storage type in the depthwise tables below
static int dt_index(int dtype) { return dtype == PCV_F32 ? 0 : (dtype == PCV_BF16 ? 1 : 2); }

// depthwise 3x3 / 5x5 (dwconv.hpp): [storage type][3x3 s1, 3x3 s2, 5x5 s1, 5x5 s2][clamp-only activations]; no dynamic LDS
#define DW_TYPE(DT)                                                                                                            \
    {{kernel_of(dwconv_kernel<DT, 3, 1, false>, 256, 0), kernel_of(dwconv_kernel<DT, 3, 1, true>, 256, 0)},                    \
     {kernel_of(dwconv_kernel<DT, 3, 2, false>, 256, 0), kernel_of(dwconv_kernel<DT, 3, 2, true>, 256, 0)},                    \
     {kernel_of(dwconv5_kernel<DT, 1, false>, 256, 0), kernel_of(dwconv5_kernel<DT, 1, true>, 256, 0)},                        \
     {kernel_of(dwconv5_kernel<DT, 2, false>, 256, 0), kernel_of(dwconv5_kernel<DT, 2, true>, 256, 0)}}
static const Kernel kDw[3][4][2] = {DW_TYPE(PCV_F32), DW_TYPE(PCV_BF16), DW_TYPE(PCV_F16)};

// depthwise MixConv (mixconv.hpp): [storage type][stride - 1][clamp-only activation][kernels - 2]; no dynamic LDS
#define MIX_KERNEL(DT, S, FAST, G) kernel_of(mixdw_kernel<DT, S, FAST, G>, 256, 0)
#define MIX_ROW(DT, S, FAST) {MIX_KERNEL(DT, S, FAST, 2), MIX_KERNEL(DT, S, FAST, 3), MIX_KERNEL(DT, S, FAST, 4), MIX_KERNEL(DT, S, FAST, 5)}
#define MIX_TYPE(DT) {{MIX_ROW(DT, 1, false), MIX_ROW(DT, 1, true)}, {MIX_ROW(DT, 2, false), MIX_ROW(DT, 2, true)}}
static const Kernel kMix[3][2][2][4] = {MIX_TYPE(PCV_F32), MIX_TYPE(PCV_BF16), MIX_TYPE(PCV_F16)};

// ghost module (ghost.hpp): [storage type][clamp-only activation]; no dynamic LDS
#define GHOST_ROW(DT) {kernel_of(ghost_dw_kernel<DT, false>, 256, 0), kernel_of(ghost_dw_kernel<DT, true>, 256, 0)}
static const Kernel kGhost[3][2] = {GHOST_ROW(PCV_F32), GHOST_ROW(PCV_BF16), GHOST_ROW(PCV_F16)};

// top-k / softmax / label rank (classify_kernel.hpp): one wave per row up to 1024 entries, four above; LDS = scratch + the row
static Kernel classify_kernel_of(int J) {
    const int lds = kClassifyRedBytes + J * 4;
    return J <= 1024 ? kernel_of(classify_kernel<64>, 64, lds) : kernel_of(classify_kernel<256>, 256, lds);
}

// ---- once per context: every instantiation with dynamic LDS gets its limit raised on the context's device, and the persistent
// kernels whose grid is a number of resident blocks get that number recorded in the context ---------------------------------------
static int enable_kernel(pcv_ctx* ctx, const Kernel& k, int* bpc) {
    HIP_TRY(ctx, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds));
    return bpc ? blocks_per_cu(ctx, k, bpc) : PCV_OK;
}
static int enable_kernels(pcv_ctx* ctx) {
    int rc = PCV_OK;
    auto on = [&](const Kernel& k, int* bpc = nullptr) {        // (.fn == nullptr: a combination that is not instantiated)
        if (rc == PCV_OK && k.fn != nullptr) rc = enable_kernel(ctx, k, bpc);
    };
    auto report = [&](const Kernel& k, int dt, int tile, int khw, int variant) {
        int nb = 0;
        if (rc == PCV_OK && k.fn != nullptr && std::getenv("PCV_AMD_DEBUG") && blocks_per_cu(ctx, k, &nb) == PCV_OK)
            std::fprintf(stderr, "[pcv] igemm dt=%d tile=%d khw=%d variant=%d: %d blocks/CU\n", dt, tile, khw, variant, nb);
    };
    static const int khws[3] = {0, 1, 9};
    for (int dt = 0; dt < 3; ++dt)
        for (int tile = 0; tile < TILE_COUNT; ++tile) {
            for (int ks = 0; ks < 3; ++ks) {
                const Kernel k = igemm_kernel(dt, dt, false, tile, khws[ks]);
                on(k, &ctx->igemm_bpc[dt][0][tile][ks]);
                report(k, dt, tile, khws[ks], 0);
            }
            // the two descriptor-driven variants (fp32 output; ragged in the input's type) share a slot: the second one's figure
            const Kernel f32out = igemm_kernel(dt, PCV_F32, true, tile, 0), same = igemm_kernel(dt, dt, true, tile, 0);
            on(f32out);
            report(f32out, dt, tile, 0, 1);
            on(same, &ctx->igemm_bpc[dt][1][tile][0]);
            report(same, dt, tile, 0, 2);
        }
    for (const auto& T : kD3Tables)
        for (int i = 0; i < T.n; ++i)
            for (int t = 0; t < 2; ++t) on(T.rows[i][t]);
    // where a slot serves both 16-bit types the launches have always used the fp16 instance's figure: bf16 is enabled only
    for (int slot = 0; slot < 3; ++slot) {
        on(gconv_kernel(PCV_BF16, slot));
        on(gconv_kernel(PCV_F16, slot), &ctx->gconv_bpc[slot]);
    }
    for (int dt = PCV_BF16; dt <= PCV_F16; ++dt)
        for (int s = 1; s <= 2; ++s)
            for (int kt = 5; kt <= 9; kt += 4) on(gconvr_kernel(dt, s, kt));
    for (int t = 0; t < 2; ++t)
        for (int s = 0; s < 2; ++s)
            for (int pbi = 0; pbi < 2; ++pbi)
                for (int wi = 0; wi < 7; ++wi) on(kGConvX[t][s][pbi][wi], (t == 1 && s == 0 && wi == 6) ? &ctx->gconvx_bpc[pbi] : nullptr);
    for (int t = 0; t < 2; ++t)
        for (int nchw = 0; nchw < 2; ++nchw)
            for (int form = 0; form < 3; ++form) on(kStem[t][nchw][form], (nchw == 0 && form == STEM_PLAIN) ? &ctx->stem_bpc[t] : nullptr);
    for (int form = 0; form < 4; ++form) {
        on(kPair[0][form]);
        on(kPair[1][form], form == PAIR_GATED ? nullptr : form == PAIR_IDCONV ? &ctx->pair_idc_bpc : &ctx->pair_bpc[form]);
    }
    for (int t = 0; t < 2; ++t)
        for (int form = 0; form < 2; ++form) on(kBnu[t][form]);
    for (int cfg = 0; cfg < 4; ++cfg)
        for (int gated = 0; gated < 2; ++gated) {
            on(wpair_launch(cfg, PCV_BF16, gated != 0).k);
            on(wpair_launch(cfg, PCV_F16, gated != 0).k, gated ? nullptr : &ctx->wpair_bpc[cfg]);
        }
    for (int dt = PCV_BF16; dt <= PCV_F16; ++dt)
        for (int s = 1; s <= 2; ++s)
            for (int e = 0; e < 2; ++e) on(mbconv_kernel(dt, s, e != 0));
    for (const MbwEntry& e : kMbw) on(mbw_kernel_of(e));
    for (const MbrEntry& e : kMbr) on(mbr_kernel_of(e));
    on(classify_kernel_of(1024));
    on(classify_kernel_of(kClassifyMaxJ));
    return rc;
}
// Shapes the wave-private kernel (mbw.hpp) runs: an expand convolution with one K step (Cin <= 32: any stride, <= 64 projected
// channels, weights in LDS) or two (Cin <= 64: stride 1, <= 64 projected channels, weights stay in L2).
// ... or, WIDE units (pcv_set_tuning("mbw_wide", 0) = off): 65..96 projected channels with two or three K steps at stride 1, on wave
// tiles of 2 pixel blocks (rb = 2) of 1 x 16 pixels.
static bool mbw_shape(int Cin, int Cout, int stride, int H, int W, int* ka_out, int* nrt_out, int* rb_out = nullptr) {
    const int ka = (Cin + 31) / 32, nrt = Cout <= 32 ? 2 : (Cout <= 64 ? 4 : 6);
    if (ka_out) *ka_out = ka;
    if (nrt_out) *nrt_out = nrt;
    if (rb_out) *rb_out = nrt == 6 ? 2 : 0;
    if (H > 250 || W > 250 || Cout > 96) return false;
    if (nrt == 6) return g_mbw_wide != 0 && stride == 1 && (ka == 2 || ka == 3);
    return ka == 1 || (ka == 2 && stride == 1 && nrt == 4);
}
// de: expand 1x1 (may be null), dd: depthwise 3x3, dp: project 1x1
static const char* mbconv_unsupported(const pcv_conv_desc* de, const pcv_conv_desc& dd, const pcv_conv_desc& dp) {
    if ((de && desc_stale(*de)) || desc_stale(dd) || desc_stale(dp)) return kStaleDesc;
    if (dd.dtype != PCV_BF16 && dd.dtype != PCV_F16) return "16-bit storage only";
    if (dd.kh != 3 || dd.kw != 3 || dd.dil_h != 1 || dd.dil_w != 1 || dd.pad_t != 1 || dd.pad_l != 1 || dd.pad_b != 1 ||
        dd.pad_r != 1 || dd.stride_h != dd.stride_w || (dd.stride_h != 1 && dd.stride_h != 2) || dd.groups != dd.Cin ||
        dd.Cin != dd.Cout || dd.has_residual || dd.out_dtype != dd.dtype || (dd.x_cpitch != 0 && dd.x_cpitch != dd.Cin) ||
        (dd.x_wpitch != 0 && dd.x_wpitch != dd.W))
        return "depthwise stage must be 3x3, pad 1, stride 1 or 2, no residual";
    const int Cmid = dd.Cin;
    if (Cmid % 8 != 0) return "expanded channels must be a multiple of 8";
    if (!plain_1x1(dp) || dp.dtype != dd.dtype || dp.Cin != Cmid || dp.Cout % 8 != 0 || dp.Cout > 96) return "project stage must be a plain 1x1 with at most 96 channels";
    // measured (MobileNetV2, batch 512): the fused unit wins on the large maps (the expanded tensor is what costs) and loses on
    // 14x14 and below / wide projections, where the three separate launches are cheap and this kernel is VALU-bound
    // the wave-private kernel (mbw.hpp: at most 32 unit inputs, one expand K step) also takes 64 projected channels and 14x14 maps
    const bool wave_tiles = de && mbw_shape(de->Cin, dp.Cout, dd.stride_h, dd.H, dd.W, nullptr, nullptr);
    if (dp.Cout > (wave_tiles ? 96 : 32)) return "fused unit only pays for narrow projections";
    const int Ho = (dd.H - 1) / dd.stride_h + 1, Wo = (dd.W - 1) / dd.stride_w + 1;
    if (dp.N != dd.N || dp.H != Ho || dp.W != Wo) return "shapes do not chain";
    if (Wo < (wave_tiles ? 14 : 24) || Ho < 8) return "map too small for the fused unit to pay";
    int ka = 0;
    if (de) {
        if (!plain_1x1(*de) || de->dtype != dd.dtype || de->Cout != Cmid || de->Cin % 8 != 0 || de->has_residual ||
            de->N != dd.N || de->H != dd.H || de->W != dd.W)
            return "expand stage must be a plain 1x1 onto the depthwise input";
        ka = (de->Cin + 31) / 32;
        if (ka > 3) return "expand stage input wider than 96 channels";
    }
    int nbuf = 0;
    if (wave_tiles) {
        if (mbw_waves(dd.stride_h, dp.Cout <= 32 ? 2 : (dp.Cout <= 64 ? 4 : 6), (Cmid + 31) / 32, 16, ka, dp.Cout > 64 ? 2 : 0) == 0)
            return "tiles do not fit the LDS budget";
    } else if (mbconv_plan(dd.stride_h, de != nullptr, ka, (Cmid + 31) / 32, (dp.Cout + 31) / 32 * 2, &nbuf).total > kMbMaxLds)
        return "weights + tiles do not fit the LDS budget";
    const long cin = de ? de->Cin : Cmid;
    if ((long)dd.N * dd.H * dd.W * cin * 2 >= (1L << 31) || (long)dd.N * Ho * Wo * dp.Cout * 2 >= (1L << 31)) return kTensorTooLarge;
    return nullptr;
}

// launch helpers (templates need C++ linkage)
// `dt` -> `ot` (dt or fp32); `radix` > 1: the split-attention squeeze over x with radix * C channels per pixel (pcv_splat_squeeze)
static void launch_mean(const void* x, void* y, int N, int HW, int C, int dt, int ot, hipStream_t s, int radix = 1) {
    dim3 grid((unsigned)N, (unsigned)((C / 8 + 511) / 512));
    for_dtype_out(dt, ot, [&](auto T, auto O) { spatial_mean_kernel<DT_OF(T), DT_OF(O)><<<grid, 512, 0, s>>>(x, y, HW, C, radix); });
}
// `pad` / `count_pad` / `ovf`: the padded pool of pcv_avgpool2d_pad (pcv_avgpool2d: no padding, no range counting)
static int launch_avg(pcv_ctx* ctx, const char* fn, const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int k, int s,
                      int dt, int ot, hipStream_t st, int pad = 0, int count_pad = 1, uint32_t* ovf = nullptr) {
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, fn, (long long)N * Ho * Wo * (C / 8), &grid)) return rc;
    for_dtype_out(dt, ot, [&](auto T, auto O) {
        avgpool_kernel<DT_OF(T), DT_OF(O)><<<grid, 256, 0, st>>>(x, y, N, H, W, C, Ho, Wo, k, s, pad, count_pad, ovf);
    });
    return launched(ctx);
}


// ---------------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------------
extern "C" {

int pcv_abi_version(void) { return PCV_ABI_VERSION; }

size_t pcv_conv_desc_size(void) { return sizeof(pcv_conv_desc); }

const char* pcv_last_error(const pcv_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

int pcv_create(pcv_ctx** out, int device) {
    if (out == nullptr) return fail(nullptr, PCV_ERR_INVALID, "pcv_create: out is NULL");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(nullptr, PCV_ERR_NO_DEVICE, "pcv_create: no HIP device visible");
    if (device < 0 || device >= count) return fail(nullptr, PCV_ERR_INVALID, "pcv_create: bad device index");
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, PCV_ERR_NO_DEVICE,
                    std::string("pcv_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    int prev = 0;
    HIP_TRY(nullptr, hipGetDevice(&prev));
    HIP_TRY(nullptr, hipSetDevice(device));
    pcv_ctx* ctx = new (std::nothrow) pcv_ctx();
    if (ctx == nullptr) return fail(nullptr, PCV_ERR_INVALID, "pcv_create: out of host memory");
    ctx->device = device;
    ctx->num_cu = prop.multiProcessorCount;
    if (const char* e = std::getenv("PCV_AMD_PERSIST")) ctx->persist_mode = std::atoi(e);
    if (const char* e = std::getenv("PCV_AMD_PERSIST_NK")) ctx->persist_max_nk = std::atoi(e);
    int rc = enable_kernels(ctx);
    if (rc == PCV_OK) {
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&ctx->ovf), 256);
        if (e == hipSuccess) e = hipMemset(ctx->ovf, 0, 256);
        if (e != hipSuccess) rc = fail(ctx, PCV_ERR_HIP, std::string("pcv_create: overflow counter: ") + hipGetErrorString(e));
    }
    if (rc != PCV_OK) {
        g_create_err = ctx->err;
        if (ctx->ovf) (void)hipFree(ctx->ovf);
        delete ctx;
        (void)hipSetDevice(prev);
        return rc;
    }
    (void)hipSetDevice(prev);
    *out = ctx;
    return PCV_OK;
}

// Tuning/debug switches (same keys as the PCV_AMD_* environment variables read by pcv_create); not part of the
// reference-facing contract. Returns PCV_ERR_INVALID for an unknown key.
static const struct { const char* key; int pcv_ctx::*field; } kTuningKeys[] = {
    {"persist", &pcv_ctx::persist_mode}, {"persist_nk", &pcv_ctx::persist_max_nk}, {"tile", &pcv_ctx::force_tile},
    {"pair_pb", &pcv_ctx::pair_pb},      {"max_blocks", &pcv_ctx::max_blocks},     {"d3x3", &pcv_ctx::use_d3x3},
    {"d3w", &pcv_ctx::use_d3w},          {"d3c", &pcv_ctx::use_d3c},               {"d3k", &pcv_ctx::use_d3k},
    {"d3i", &pcv_ctx::use_d3i},          {"d1i", &pcv_ctx::use_d1i},               {"p1r", &pcv_ctx::use_p1r},
    {"head", &pcv_ctx::use_head},        {"stem32", &pcv_ctx::use_stem32},         {"d1x1", &pcv_ctx::use_d1x1},
    {"gconvr", &pcv_ctx::use_gconvr},    {"mbw", &pcv_ctx::use_mbw},               {"mbr", &pcv_ctx::use_mbr},
    {"mbr_xl", &pcv_ctx::use_mbr_xl},    {"dw_th", &pcv_ctx::dw_th},               {"dw_flags", &pcv_ctx::dw_flags},
    {"wstat", &pcv_ctx::use_wstat},      {"bnu_band", &pcv_ctx::bnu_band},         {"gconvx", &pcv_ctx::use_gconvx},
};
int pcv_set_tuning(pcv_ctx* ctx, const char* key, int value) {
    if (!ctx || !key) return PCV_ERR_INVALID;
    const std::string k(key);
    for (const auto& t : kTuningKeys)
        if (k == t.key) {
            ctx->*t.field = value;
            return PCV_OK;
        }
    if (k == "mbw_wide") g_mbw_wide = value;                // these three: process-wide (see their definition)
    else if (k == "wpair") g_wpair_mask = value;
    else if (k == "bnu") g_bnu = value;
    else if (k == "dbg") {
#ifdef PCV_DBG_FLAGS
        ctx->dbg_flags = value;
#else
        if (value != 0)
            return fail(ctx, PCV_ERR_INVALID, "pcv_set_tuning: \"dbg\" (timing experiments that produce wrong results) needs a -DPCV_DBG_FLAGS build");
#endif
    }
    else if (k == "dbg_lo") ctx->dbg_ptr = (ctx->dbg_ptr & 0xFFFFFFFF00000000ull) | (unsigned)value;
    else if (k == "dbg_hi") ctx->dbg_ptr = (ctx->dbg_ptr & 0xFFFFFFFFull) | ((unsigned long long)(unsigned)value << 32);
    else return fail(ctx, PCV_ERR_INVALID, "pcv_set_tuning: unknown key " + k);
    return PCV_OK;
}

int pcv_destroy(pcv_ctx* ctx) {
    if (ctx && ctx->ovf) {
        DeviceGuard device_guard(ctx->device);
        (void)hipFree(ctx->ovf);
    }
    delete ctx;
    return PCV_OK;
}

// ---- fp16 range guard ---------------------------------------------------------------------------------------
int pcv_fp16_guard_begin(pcv_ctx* ctx, unsigned* slot, void* stream) {
    PCV_ENTER(ctx);
    if (!slot) return fail(ctx, PCV_ERR_INVALID, "pcv_fp16_guard_begin: slot is NULL");
    f16_guard_begin_kernel<<<1, 1, 0, (hipStream_t)stream>>>(ctx->ovf, slot);
    return launched(ctx);
}

int pcv_fp16_guard_end(pcv_ctx* ctx, const unsigned* slot, float* y, long count, void* stream) {
    PCV_ENTER(ctx);
    if (!slot || !y || count <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_fp16_guard_end: bad argument");
    const unsigned grid = (unsigned)std::min<long>((count + 255) / 256, 1024);
    f16_guard_end_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(ctx->ovf, slot, y, count);
    return launched(ctx);
}

// ---- RCCL helpers (resolved at run time: no link-time dependency) ----------------------------------------------
extern "C++" {
namespace {
typedef int (*nccl_group_fn)(void);
typedef int (*nccl_bcast_fn)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_gather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
typedef const char* (*nccl_err_fn)(int);
struct RcclApi {
    nccl_group_fn group_start = nullptr, group_end = nullptr;
    nccl_bcast_fn broadcast = nullptr;
    nccl_gather_fn allgather = nullptr;
    nccl_err_fn error_string = nullptr;
    bool ok = false;
};
const RcclApi& rccl_api() {
    static const RcclApi api = [] {
        RcclApi a;
        // the librccl this process already has (by SONAME: also finds one that PyTorch loaded privately), else load one
        void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
        if (!h) h = dlopen("librccl.so.1", RTLD_NOW);
        if (!h) h = dlopen("librccl.so", RTLD_NOW);
        if (!h) return a;
        a.group_start = reinterpret_cast<nccl_group_fn>(dlsym(h, "ncclGroupStart"));
        a.group_end = reinterpret_cast<nccl_group_fn>(dlsym(h, "ncclGroupEnd"));
        a.broadcast = reinterpret_cast<nccl_bcast_fn>(dlsym(h, "ncclBroadcast"));
        a.allgather = reinterpret_cast<nccl_gather_fn>(dlsym(h, "ncclAllGather"));
        a.error_string = reinterpret_cast<nccl_err_fn>(dlsym(h, "ncclGetErrorString"));
        a.ok = a.group_start && a.group_end && a.broadcast && a.allgather;
        return a;
    }();
    return api;
}
const int kNcclUint8 = 1;        // ncclUint8 / ncclChar = 0 or 1 in nccl.h: both are one byte per element
int rccl_fail(pcv_ctx* ctx, const char* what, int rc) {
    const RcclApi& R = rccl_api();
    return fail(ctx, PCV_ERR_HIP, std::string(what) + ": " + (R.error_string ? R.error_string(rc) : "RCCL error") + " (" + std::to_string(rc) + ")");
}
}  // namespace
}  // extern "C++"

int pcv_rccl_available(void) { return rccl_api().ok ? 1 : 0; }

int pcv_rccl_broadcast(pcv_ctx* ctx, void* comm, void* const* bufs, const size_t* bytes, int count, int root, void* stream) {
    PCV_ENTER(ctx);
    if (!comm || !bufs || !bytes || count <= 0 || root < 0) return fail(ctx, PCV_ERR_INVALID, "pcv_rccl_broadcast: bad argument");
    for (int i = 0; i < count; ++i)
        if (!bufs[i] || bytes[i] == 0) return fail(ctx, PCV_ERR_INVALID, "pcv_rccl_broadcast: NULL or empty buffer");
    const RcclApi& R = rccl_api();
    if (!R.ok) return fail(ctx, PCV_ERR_INVALID, "pcv_rccl_broadcast: no RCCL in this process (librccl.so.1 not found)");
    int rc = R.group_start();
    if (rc != 0) return rccl_fail(ctx, "ncclGroupStart", rc);
    for (int i = 0; i < count && rc == 0; ++i) rc = R.broadcast(bufs[i], bufs[i], bytes[i], kNcclUint8, root, comm, (hipStream_t)stream);
    const int rc_end = R.group_end();
    if (rc != 0) return rccl_fail(ctx, "ncclBroadcast", rc);
    if (rc_end != 0) return rccl_fail(ctx, "ncclGroupEnd", rc_end);
    return PCV_OK;
}

int pcv_rccl_allgather(pcv_ctx* ctx, void* comm, const void* send, void* recv, size_t bytes_per_rank, void* stream) {
    PCV_ENTER(ctx);
    if (!comm || !send || !recv || bytes_per_rank == 0) return fail(ctx, PCV_ERR_INVALID, "pcv_rccl_allgather: bad argument");
    const RcclApi& R = rccl_api();
    if (!R.ok) return fail(ctx, PCV_ERR_INVALID, "pcv_rccl_allgather: no RCCL in this process (librccl.so.1 not found)");
    const int rc = R.allgather(send, recv, bytes_per_rank, kNcclUint8, comm, (hipStream_t)stream);
    if (rc != 0) return rccl_fail(ctx, "ncclAllGather", rc);
    return PCV_OK;
}

int pcv_fp16_overflow_count(pcv_ctx* ctx, unsigned* count, void* stream) {
    PCV_ENTER(ctx);
    if (!count) return fail(ctx, PCV_ERR_INVALID, "pcv_fp16_overflow_count: count is NULL");
    HIP_TRY(ctx, hipMemcpyAsync(count, ctx->ovf, sizeof(unsigned), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIP_TRY(ctx, hipStreamSynchronize((hipStream_t)stream));
    return PCV_OK;
}

// ---- layout ------------------------------------------------------------------------------------------------
int pcv_nchw_to_nhwc(pcv_ctx* ctx, const float* x, void* y, int N, int C, int H, int W, int cpitch, int wpitch,
                     int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || cpitch < C || wpitch < W || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_nchw_to_nhwc: bad argument");
    if (!(cpitch == 4 || cpitch % 8 == 0) && !(dtype == PCV_F32 && cpitch % 4 == 0))
        return fail(ctx, PCV_ERR_INVALID, "pcv_nchw_to_nhwc: cpitch must be 4 or a multiple of 8");
    dim3 grid(0, (unsigned)((cpitch + 7) / 8));
    if (int rc = flat_grid(ctx, "pcv_nchw_to_nhwc", (long long)N * H * wpitch, &grid.x)) return rc;
    hipStream_t s = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { nchw_to_nhwc_kernel<DT_OF(T)><<<grid, 256, 0, s>>>(x, y, N, C, H, W, cpitch, wpitch, ctx->ovf); });
    return launched(ctx);
}

int pcv_nhwc_to_nchw(pcv_ctx* ctx, const void* x, float* y, int N, int C, int H, int W, int cpitch, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (cpitch <= 0) cpitch = C;
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || cpitch < C || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_nhwc_to_nchw: bad argument");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_nhwc_to_nchw", (long long)N * C * H * W, &grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { nhwc_to_nchw_kernel<DT_OF(T)><<<grid, 256, 0, s>>>(x, y, N, C, H, W, cpitch); });
    return launched(ctx);
}

// ---- weights -----------------------------------------------------------------------------------------------
int pcv_conv_packed_bytes(const pcv_conv_desc* d, size_t* bytes) {
    if (!d || !bytes) return PCV_ERR_INVALID;
    ConvPlan P;
    if (plan_conv(*d, P, false) != nullptr) return PCV_ERR_INVALID;
    *bytes = P.total_bytes;
    return PCV_OK;
}

int pcv_conv_pack(pcv_ctx* ctx, const pcv_conv_desc* d, const float* w, void* packed, void* stream) {
    PCV_ENTER(ctx);
    if (!d || !w || !packed) return fail(ctx, PCV_ERR_INVALID, "pcv_conv_pack: NULL argument");
    if (!aligned16(packed)) return fail(ctx, PCV_ERR_INVALID, "pcv_conv_pack: packed buffer must be 16-byte aligned");
    ConvPlan P;
    const char* why = plan_conv(*d, P, true);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_conv_pack: ") + why);
    hipStream_t s = (hipStream_t)stream;
    if (P.stem) {
        const int total = d->kh * 64 * 32;
        for_dtype16(d->dtype, [&](auto T) {
            pack_stem_kernel<DT_OF(T)><<<(total + 255) / 256, 256, 0, s>>>(w, packed, d->Cout, d->Cin, d->kh, d->kw, d->pad_l & 1);
        });
        return launched(ctx);
    }
    unsigned grid = 0, ggrid = 0;
    if (int rc = flat_grid(ctx, "pcv_conv_pack", (long long)P.ngb * P.wrows * P.Kpad, &grid)) return rc;
    if (int rc = flat_grid(ctx, "pcv_conv_pack", P.gconv ? (long long)(d->Cin / 16) * P.gconv_kt * 16 * 32 : 0, &ggrid)) return rc;
    if (P.gconvx)
        if (int rc = flat_grid(ctx, "pcv_conv_pack", gconvx_packed_elems(d->groups, P.Cg_in), &ggrid)) return rc;
    // load-time only: synchronous uploads of the two small host-built tables
    uint32_t* ksrc_dev = nullptr;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&ksrc_dev), P.ksrc.size() * sizeof(uint32_t)));
    hipError_t e = hipMemcpy(ksrc_dev, P.ksrc.data(), P.ksrc.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(packed, P.ktab.data(), P.ktab.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(ksrc_dev);
        return fail(ctx, PCV_ERR_HIP, std::string("pcv_conv_pack: table upload: ") + hipGetErrorString(e));
    }
    PackParams pp;
    pp.w = w;
    pp.out = static_cast<char*>(packed) + P.ktab_bytes;
    pp.ksrc = ksrc_dev;
    pp.ngb = P.ngb;
    pp.wrows = P.wrows;
    pp.Kpad = P.Kpad;
    pp.cout_blk = P.cout_blk;
    pp.cin_blk = d->groups == 1 ? 0 : P.cin_blk;
    pp.Cg_in = P.Cg_in;
    pp.Cg_out = P.Cg_out;
    pp.khkw = d->kh * d->kw;
    for_dtype(d->dtype, [&](auto T) { pack_conv_kernel<DT_OF(T)><<<grid, 256, 0, s>>>(pp); });
    if (P.gconv) {
        void* gout = static_cast<char*>(packed) + P.gconv_off;
        for_dtype16(d->dtype, [&](auto T) {
            if (P.gconv_kt == 9) pack_gconv32_kernel<DT_OF(T)><<<ggrid, 256, 0, s>>>(w, gout, d->Cin);
            else pack_gconv_kernel<DT_OF(T)><<<ggrid, 256, 0, s>>>(w, gout, d->Cin, P.Cg_in);
        });
    }
    if (P.gconvx) {
        void* gout = static_cast<char*>(packed) + P.gconvx_off;
        for_dtype16(d->dtype, [&](auto T) { pack_gconvx_kernel<DT_OF(T)><<<ggrid, 256, 0, s>>>(w, gout, d->groups, P.Cg_in); });
    }
    if (P.d3i || P.d1i) {
        const int total = (int)((P.total_bytes - P.d3i_off) / 16);
        pack_d3i_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(reinterpret_cast<const u32x4*>(pp.out),
                                                                        reinterpret_cast<u32x4*>(static_cast<char*>(packed) + P.d3i_off), P.Kpad, total);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    (void)hipFree(ksrc_dev);
    if (e != hipSuccess) return fail(ctx, PCV_ERR_HIP, std::string("pcv_conv_pack: ") + hipGetErrorString(e));
    return PCV_OK;
}

static const char* check_dw(const pcv_conv_desc& d) {
    if (desc_stale(d)) return kStaleDesc;
    if (!dtype_ok(d.dtype) || d.out_dtype != d.dtype) return "depthwise: out_dtype must equal dtype";
    if (d.groups != d.Cin || d.Cin != d.Cout) return "depthwise: needs groups == Cin == Cout";
    if (d.Cin % 8 != 0) return "depthwise: channels must be a multiple of 8";
    if (d.kh != d.kw || (d.kh != 3 && d.kh != 5)) return "depthwise: only 3x3 and 5x5";
    if (d.stride_h != d.stride_w || (d.stride_h != 1 && d.stride_h != 2)) return "depthwise: stride 1 or 2";
    if (d.dil_h != 1 || d.dil_w != 1) return "depthwise: dilation unsupported";
    if (d.x_cpitch > 0 && d.x_cpitch != d.Cin) return "depthwise: padded channel pitch unsupported";
    if (d.x_wpitch > 0 && d.x_wpitch != d.W) return "depthwise: padded row pitch unsupported";
    if (d.y_cpitch > 0 && d.y_cpitch != d.Cout) return "depthwise: y must be dense";
    return nullptr;
}

// packed depthwise blob: the taps [kh * kw][C] (what the depthwise kernels read), then - 16-bit 3x3 only - the compressed diagonal
// fragments of the sparse matrix instruction for the fused inverted-residual kernel (pack_dw_sparse_kernel, csrc/mbr.hpp)
static size_t dw_taps_bytes(const pcv_conv_desc& d) { return (((size_t)d.kh * d.kw * d.Cin * esize(d.dtype)) + 15) & ~(size_t)15; }
static size_t dw_sparse_bytes(const pcv_conv_desc& d) {
    return (d.kh == 3 && d.dtype != PCV_F32) ? (size_t)((d.Cin + 31) / 32) * 6 * 1024 : 0;
}
int pcv_dwconv_packed_bytes(const pcv_conv_desc* d, size_t* bytes) {
    if (!d || !bytes || check_dw(*d)) return PCV_ERR_INVALID;
    *bytes = dw_taps_bytes(*d) + dw_sparse_bytes(*d);
    return PCV_OK;
}

int pcv_dwconv_pack(pcv_ctx* ctx, const pcv_conv_desc* d, const float* w, void* packed, void* stream) {
    PCV_ENTER(ctx);
    if (!d || !w || !packed) return fail(ctx, PCV_ERR_INVALID, "pcv_dwconv_pack: NULL argument");
    const char* why = check_dw(*d);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_dwconv_pack: ") + why);
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_dwconv_pack", (long long)d->Cin * d->kh * d->kw, &grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    for_dtype(d->dtype, [&](auto T) { pack_dw_kernel<DT_OF(T)><<<grid, 256, 0, s>>>(w, packed, d->Cin, d->kh * d->kw); });
    if (dw_sparse_bytes(*d) != 0) {
        const int nChunks = (d->Cin + 31) / 32;
        pack_dw_sparse_kernel<<<(unsigned)((nChunks * 6 * 64 + 255) / 256), 256, 0, s>>>(
            static_cast<const uint16_t*>(packed), reinterpret_cast<u32x4*>(static_cast<char*>(packed) + dw_taps_bytes(*d)), d->Cin, nChunks);
    }
    return launched(ctx);
}

int pcv_bn_fold(pcv_ctx* ctx, int C, const float* gamma, const float* beta, const float* mean, const float* var,
                float eps, const float* conv_bias, float* scale, float* shift, void* stream) {
    PCV_ENTER(ctx);
    if (C <= 0 || !scale || !shift) return fail(ctx, PCV_ERR_INVALID, "pcv_bn_fold: bad argument");
    const bool any = gamma || beta || mean || var;
    const bool all = gamma && beta && mean && var;
    if (any && !all) return fail(ctx, PCV_ERR_INVALID, "pcv_bn_fold: gamma/beta/mean/var must be all set or all NULL");
    bn_fold_kernel<<<(C + 255) / 256, 256, 0, (hipStream_t)stream>>>(C, gamma, beta, mean, var, eps, conv_bias, scale, shift);
    return launched(ctx);
}

// ---- hot path ----------------------------------------------------------------------------------------------
static int pool_out(int in, int k, int s, int p, int ceil_mode);
static void launch_se_fc(const float* in, const float* w, const float* b, float* out, int N, int K, int J, int act, hipStream_t st);

// ---------------------------------------------------------------------------------------------------------
// One convolution launch = route (which kernel family, which tile shape: a pure function of the descriptor, the plan and the
// context's switches) + that family's launcher (parameter block, grid, launch). conv2d_impl validates, routes, dispatches.
// ---------------------------------------------------------------------------------------------------------
enum ConvKernel {
    CK_STEM,        // stem_conv.hpp: Cin <= 4, stride 2 (+ fused max-pool, + fp32 NCHW input)
    CK_GCONV_ROWS,  // gconv3x3r.hpp: grouped 3x3, stride 2 or 32 channels per group
    CK_GCONV_FLAT,  // gconv3x3.hpp: grouped 3x3, stride 1, 4 / 8 / 16 channels per group
    CK_GCONVX,      // gconvx.hpp: grouped 3x3 at the widths and channel counts the two above do not take (RegNet)
    CK_D3I,         // d3i_conv.hpp: dense 3x3 / s1 / p1, 16 bit, 256 input channels on maps up to 14 x 14 or 512 up to 7 x 7 (image(s) in LDS, weights straight to registers)
    CK_D1I,         // d1i_conv.hpp: 1x1 / s1, 16 bit, 1024 / 2048 input channels (activations streamed through LDS, weights straight to registers)
    CK_D3K,         // d3k_conv.hpp: dense 3x3 / s1 / p1, 16 bit, 128 input channels on 28-wide maps (weights in registers / AGPRs)
    CK_D3C,         // d3c_conv.hpp: dense 3x3 / s1 / p1, 16 bit, 64 input channels on 56-wide maps (weights in registers)
    CK_D3W,         // d3w_conv.hpp: dense 3x3 / s1 / p1, 16 bit, large tiles (eight self-loading waves)
    CK_D3Q,         // d3q_conv.hpp: dense 3x3 / s1 / p1, 16 bit
    CK_P1R,         // p1r_conv.hpp: 1x1 with 256 / 512 input channels, weights in registers, epilogue under the next pixel block's MFMAs
    CK_D3Q_1X1,     // d3q_conv.hpp in its 1x1 mode: K-heavy pointwise layers
    CK_HEAD,        // head_gemm.hpp: fp32 dense layer on a 1x1 map (classifier)
    CK_IGEMM        // igemm_conv.hpp: everything else
};
struct ConvRoute {
    ConvKernel kernel = CK_IGEMM;
    int shape = -1;             // CK_D3Q / CK_D3Q_1X1: index into kD3 / kD1
    GConvRPlan rows{};          // CK_GCONV_ROWS
    GConvXPlan xrows{};         // CK_GCONVX
    int tile = TILE_C128, khw = 0;      // CK_IGEMM: tile configuration, tap mode (0 table, 1 = 1x1, 9 = 3x3)
    bool special = false;       // CK_IGEMM: ragged channel count or fp32 output (the descriptor-driven 128 x 128 variants)
};
// what a launch addresses besides the descriptor
struct ConvArgs {
    const void* x; const void* packed; const float* scale; const float* shift; const void* residual; void* y;
    const float* gate; hipStream_t stream;
    bool pool;                  // the MaxPool2d(3, 2, 1) of the init block fused behind the stem convolution (pcv_conv2d_maxpool_fused)
    bool x_nchw;                // the stem reads the fp32 NCHW image itself (pcv_conv2d_nchw_stem_fused); `d` still describes the padded NHWC4 view
};
// sizes every launcher needs
struct ConvGeom {
    int cpitch, wpitch;
    unsigned long long xbytes, M64;
    bool sliced_y;
};

// Tile configuration of the generic kernel for a plan (tests/tools/sweep_1x1_tiles.py has the measurements behind the rules).
static void route_igemm(const pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, ConvRoute& R) {
    const bool ragged = (d->Cout % 8 != 0) || (P.cout_blk % 8 != 0);
    int tile;
    if (ragged || d->out_dtype != d->dtype) tile = TILE_C128;
    else if (P.cout_blk <= 32) tile = TILE_C32;
    else if (P.cout_blk <= 64) tile = TILE_C64;
    else if (P.cout_blk <= 128) tile = TILE_C128;
    else if (P.cout_blk <= 256) tile = (d->kh * d->kw > 1) ? TILE_C128 : TILE_C256;   // 256x64 only pays for HBM-bound 1x1 (reads x once)
    else tile = TILE_C128;
    R.special = ragged || d->out_dtype != d->dtype;
    int khw = 0;
    if (!R.special && !P.pair && d->dil_h == 1 && d->dil_w == 1) {
        if (d->kh == 1 && d->kw == 1 && d->pad_t == 0 && d->pad_l == 0 && d->pad_b == 0 && d->pad_r == 0) khw = 1;
        else if (d->kh == 3 && d->kw == 3 && P.cin_blk % (8 * P.CE) == 0) khw = 9;
    }
    if (khw == 1) {
        // 1x1 reductions (many K-steps into few channels) run best on the half-height tiles (3 blocks per CU); the 256-channel
        // tile only pays when the input is narrow (it reads x once)
        if (tile == TILE_C64 && d->Cin >= 256) tile = TILE_C64S;
        else if (tile == TILE_C128 && P.cout_blk <= 128 && d->Cin >= 512) tile = TILE_C128S;
        else if (tile == TILE_C256 && d->Cin > 128) tile = TILE_C128;
        // Swish / sigmoid epilogues are VALU-bound (two quarter-rate transcendentals per element: the 16 -> 96 expand layer of
        // EfficientNet at 112x112 takes 384 us with Swish against 215 us with ReLU6): with one or two K-steps per tile the
        // half-height tiles (3 blocks per CU) overlap that epilogue with other blocks' loads - 13-26 % faster in a tile sweep.
        // Of the two, the one that pads fewer channel rows; ties go to the 128-row tile (x is re-read less).
        if ((d->act == PCV_ACT_SWISH || d->act == PCV_ACT_SIGMOID) && P.nk <= 2 && P.ngb == 1 && !d->has_residual) {
            const int pad64 = round_up(P.cout_blk, 64), pad128 = round_up(P.cout_blk, 128);
            tile = pad64 < pad128 ? TILE_C64S : TILE_C128S;
        }
    }
    if (ctx->force_tile >= 0 && ctx->force_tile < TILE_COUNT && !R.special && (ctx->force_tile < TILE_C64S || khw == 1))
        tile = ctx->force_tile;
    R.tile = tile;
    R.khw = khw;
}

// The shape classes (channels per group, stride, map width) on which gconvx.hpp measured FASTER than the generic kernel at batch 256
// (five interleaved runs against the commit before it, slowest against fastest: profiles/experiments/gconvx_kernel.md). Measured at
// 8, 24, 48 and 56 channels per group, then at 16, 40 and 64 with 16 following 8 / 24 and 40 following 48 (both confirmed). Lost and
// sent back to the generic kernel: 48 (and 40) per group at stride 2 on 28 .. 56-wide maps (six units on four waves), 56 per group at
// stride 2 on maps wider than 56 and at stride 1 on maps wider than 28 (the three-group layers of regnety080's first stage), and 64
// per group everywhere (regnety040: slower on five of its six layers, 3 % faster on one) - its instantiation stays for the next attempt.
static bool gconvx_pays(int cg, int stride, int W) {
    if (cg <= 24) return true;
    if (cg <= 48) return !(stride == 2 && W >= 28 && W <= 56);
    if (cg > 56) return false;
    return !((stride == 2 && W > 56) || (stride == 1 && W > 28));
}

// Why a plain launch of `d` does not run on gconvx.hpp (nullptr: it does; *out then holds its tile). gconv_ok's launch conditions:
// no gate, no residual, no post_act, dense pitches, no sliced output, tensors below 2 GiB.
static const char* gconvx_launch_why(const pcv_conv_desc& d, const ConvPlan& P, const ConvGeom& G, bool gated, GConvXPlan* out) {
    if (!P.gconvx) {
        if (P.gconv) return "the shape belongs to the ResNeXt kernels (C % 64 == 0, 4 / 8 / 16 / 32 channels per group: gconv3x3.hpp, gconv3x3r.hpp)";
        if (P.ES != 2 || d.out_dtype != d.dtype) return "16-bit storage only, out_dtype == dtype";
        if (d.groups <= 1 || d.kh != 3 || d.kw != 3 || d.Cin != d.Cout) return "needs a grouped 3x3 convolution with Cin == Cout";
        if (d.dil_h != 1 || d.dil_w != 1 || d.pad_t != 1 || d.pad_l != 1 || d.pad_b != 1 || d.pad_r != 1) return "needs padding 1 and dilation 1";
        if (d.stride_h != d.stride_w || (d.stride_h != 1 && d.stride_h != 2)) return "stride 1 or 2 only";
        return "channels per group must be 8, 16, 24, 40, 48, 56 or 64";
    }
    if (gated) return "a gated launch runs on the generic kernel";
    if (d.has_residual || d.post_act != PCV_ACT_NONE) return "a residual / post_act launch runs on the generic kernel";
    if (G.sliced_y) return "a sliced output (y_cpitch) runs on the generic kernel";
    if (G.cpitch != d.Cin || G.wpitch != d.W) return "padded input pitches run on the generic kernel";
    if (G.M64 * (unsigned long long)d.Cin * 2ull >= 0x80000000ull || !in_window(G.xbytes)) return kTensorTooLarge;
    GConvXPlan g;
    if (!plan_gconvx(d.stride_h, d.H, d.W, P.Ho, P.Wo, d.groups, P.Cg_in, g))
        return "the map is odd at stride 2 or wider than 112 columns";
    if (!gconvx_pays(P.Cg_in, d.stride_h, d.W)) return "measured slower than the generic kernel on this shape class (channels per group, stride, map width)";
    if (out) *out = g;
    return nullptr;
}

static ConvRoute route_conv(const pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A) {
    ConvRoute R;
    if (P.stem) { R.kernel = CK_STEM; return R; }
    const bool gconv_ok = P.gconv && !A.gate && !G.sliced_y && !d->has_residual && d->post_act == PCV_ACT_NONE && G.cpitch == d->Cin &&
                          G.wpitch == d->W && G.M64 * (unsigned long long)d->Cin * 2ull < 0x80000000ull;
    // stride 2 (even maps) or 32 channels per group: whole output rows per tile
    if (gconv_ok && ctx->use_gconvr != 0 && (d->stride_h == 2 || P.gconv_kt == 9) &&
        plan_gconvr(d->stride_h, d->H, d->W, P.Ho, P.Wo, R.rows)) { R.kernel = CK_GCONV_ROWS; return R; }
    if (gconv_ok && d->stride_h == 1 && P.gconv_kt == 5 && d->W <= 63) { R.kernel = CK_GCONV_FLAT; return R; }
    // the group widths and channel counts the two kernels above were not built for (P.gconv false), under the same launch conditions;
    // "gconvr" 0 switches this kernel off too (tests pin the generic kernel with it)
    if (ctx->use_gconvx != 0 && ctx->use_gconvr != 0 && gconvx_launch_why(*d, P, G, A.gate != nullptr, &R.xrows) == nullptr) {
        R.kernel = CK_GCONVX;
        return R;
    }
    const bool clamp_acts = d->act <= PCV_ACT_RELU6 && d->post_act <= PCV_ACT_RELU6;       // the 8-wave kernel's branch-free epilogue
    if (P.conv3 && !A.gate && ctx->use_d3x3 != 0 && d->dtype != PCV_F32 && clamp_acts && A.scale && A.shift &&
        G.M64 * (unsigned long long)d->Cout * 2ull < 0x80000000ull &&
        G.xbytes + 2ull * (unsigned long long)d->W * d->Cin * 2ull < 0x80000000ull) {
        // 64 input channels on a 56-wide map (ResNet stage 1): 4-row tiles of one image per 64-channel tile; automatic choice from
        // two tiles per CU up (below that the 6-row patch prologue is not amortised)
        if (ctx->use_d3c != 0 && (ctx->use_d3x3 < 0 || ctx->use_d3c > 0) && (ctx->use_d3w <= 0 || ctx->use_d3c > 0) && d->Cin == D3CCfg::BM &&
            d->W == D3CCfg::W && G.cpitch == d->Cin && G.wpitch == d->W) {
            const long long tiles = (long long)((d->Cout + 63) / 64) * d->N * ((d->H + D3CCfg::ROWS - 1) / D3CCfg::ROWS);
            if (ctx->use_d3c > 0 || tiles >= 2ll * block_slots(ctx, 1)) { R.kernel = CK_D3C; return R; }
        }
        // 128 input channels on a 28-wide map (ResNet stage 2): 4-row tiles of one image per 128-channel tile, from two tiles per CU up
        if (ctx->use_d3k != 0 && (ctx->use_d3x3 < 0 || ctx->use_d3k > 0) && (ctx->use_d3w <= 0 || ctx->use_d3k > 0) && d->Cin == D3KCfg::CIN &&
            d->W == D3KCfg::W && G.cpitch == d->Cin && G.wpitch == d->W) {
            const long long tiles = (long long)((d->Cout + D3KCfg::BM - 1) / D3KCfg::BM) * d->N * ((d->H + D3KCfg::ROWS - 1) / D3KCfg::ROWS);
            if (ctx->use_d3k > 0 || tiles >= 2ll * block_slots(ctx, 1)) { R.kernel = CK_D3K; return R; }
        }
        // 256 input channels on a map of up to 14 x 14 (ResNet stage 3): one image x 256 channels per block; automatic choice for (almost)
        // full 13-block images from three quarters of a round of the CUs up (rocprofv3, batch 256 / 128: 47.6 / 39.9 us against d3w 59.0 /
        // d3q 34.9 - a block takes ~40 us however few there are)
        // 512 input channels on a map of up to 7 x 7 (stage 4): two images x 256 channels per block
        const int d3i_maxw = d->Cin == 256 ? D3ICfgT<256>::MAXW : D3ICfgT<512>::MAXW, d3i_nimg = d->Cin == 256 ? 1 : 2;
        if (P.d3i && ctx->use_d3i != 0 && (ctx->use_d3x3 < 0 || ctx->use_d3i > 0) && (ctx->use_d3w <= 0 || ctx->use_d3i > 0) &&
            d->H <= d3i_maxw && d->W <= d3i_maxw && G.cpitch == d->Cin && G.wpitch == d->W) {
            const long long tiles = (long long)((d->Cout + D3ICfg::BM - 1) / D3ICfg::BM) * ((d->N + d3i_nimg - 1) / d3i_nimg);
            // (almost) full pixel blocks: more than 11 of 13 / 5 of 7 blocks' worth of pixels
            const bool full = d3i_nimg * d->H * d->W > 16 * ((d->Cin == 256 ? D3ICfgT<256>::NBLK : D3ICfgT<512>::NBLK) - 1) - 16;
            if (ctx->use_d3i > 0 || (full && 4 * tiles >= 3ll * ctx->num_cu)) { R.kernel = CK_D3I; return R; }
        }
        if (ctx->use_d3w != 0 && (ctx->use_d3x3 < 0 || ctx->use_d3w > 0)) {       // ("d3x3" forced to a shape: that kernel, for its tests)
            R.shape = ctx->use_d3w > 0 ? std::min(ctx->use_d3w - 1, kD3WCount - 1)
                                       : pick_d3w((long long)G.M64, d->Cout, (long long)block_slots(ctx, 1));
            if (R.shape >= 0) { R.kernel = CK_D3W; return R; }
        }
        R.shape = ctx->use_d3x3 > 0 ? std::min(ctx->use_d3x3 - 1, kD3Count - 1)
                                    : pick_d3x3((long long)G.M64, d->Cout, P.nk, (long long)ctx->num_cu);
        if (R.shape >= 0) { R.kernel = CK_D3Q; return R; }
    }
    if (ctx->use_d1x1 != 0 && !A.gate && !P.pair && d->dtype != PCV_F32 && d->out_dtype == d->dtype && d->kh == 1 && d->kw == 1 &&
        d->stride_h == d->stride_w && d->stride_h <= 2 && d->pad_t == 0 && d->pad_l == 0 && d->pad_b == 0 && d->pad_r == 0 && d->groups == 1 &&
        G.cpitch == d->Cin && G.wpitch == d->W && d->Cin % 64 == 0 && d->Cout % 8 == 0 && clamp_acts && A.scale && A.shift &&
        G.M64 * (unsigned long long)d->Cout * 2ull < 0x80000000ull) {
        // 1024 / 2048 input channels at stride 1: 208-pixel x 256-channel blocks with the weights straight from L2
        if (P.d1i && ctx->use_d1i != 0 && (ctx->use_d1x1 < 0 || ctx->use_d1i > 0) && G.xbytes < 0x80000000ull) {
            const long long tiles = ((long long)G.M64 + D1ICfgT<1024>::BP - 1) / D1ICfgT<1024>::BP * ((d->Cout + 255) / 256);
            // automatic: from 1024 input channels, without a skip tensor (its epilogue is exposed: 512 -> 1024 + skip 109 against p1r's 74 us,
            // 1024 -> 2048 + skip at 7 x 7 equal), from three quarters of a round of the CUs (2048 -> 512 at 7 x 7: 122 tiles, 47 against 37 us)
            if (ctx->use_d1i > 0 || (d->Cin >= 1024 && !d->has_residual && 4 * tiles >= 3ll * ctx->num_cu)) { R.kernel = CK_D1I; return R; }
        }
        // 256 / 512 input channels: the kernel that keeps the weights in registers, where its tiles fill the chip and (almost) every
        // wave of a channel group has channels to compute
        if (ctx->use_p1r != 0 && (ctx->use_d1x1 < 0 || ctx->use_p1r > 0) && (d->Cin == 256 || d->Cin == 512) && G.xbytes < 0x80000000ull) {
            // 256 input channels: 64 channels per wave (groups of 512) unless the layer has a skip tensor (whose pieces only fit beside 32
            // channels' weights) or too few channels for 3/4 of such a group
            const int shape = d->Cin == 512 ? 1 : ((d->has_residual || d->Cout < 384) ? 2 : 0);
            const Kernel& S = kP1R[shape][0];
            const long long groups = (d->Cout + S.BM - 1) / S.BM, tiles = ((long long)G.M64 + S.BP - 1) / S.BP * groups;
            if (ctx->use_p1r > 0 || (d->Cout * 4 >= groups * S.BM * 3 && tiles >= 2ll * block_slots(ctx, 1))) {
                R.kernel = CK_P1R;
                R.shape = shape;
                return R;
            }
        }
        R.shape = ctx->use_d1x1 > 0 ? std::min(ctx->use_d1x1 - 1, kD1Count - 1)
                                    : pick_d1x1((long long)G.M64, d->Cout, d->Cin, (long long)block_slots(ctx, 1));
        if (R.shape >= 0) { R.kernel = CK_D3Q_1X1; return R; }
    }
    if (ctx->use_head && d->dtype == PCV_F32 && d->out_dtype == PCV_F32 && d->kh == 1 && d->kw == 1 && d->H == 1 && d->W == 1 &&
        P.Ho == 1 && P.Wo == 1 && d->pad_t == 0 && d->pad_l == 0 && d->pad_b == 0 && d->pad_r == 0 && d->groups == 1 && !A.gate &&
        !d->has_residual && d->post_act == PCV_ACT_NONE && d->Cin % 16 == 0) { R.kernel = CK_HEAD; return R; }
    route_igemm(ctx, d, P, R);
    return R;
}

static int launch_stem(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A) {
    const bool pool = A.pool, x_nchw = A.x_nchw;
    StemParams q;
    q.x = A.x; q.w = A.packed; q.y = A.y; q.scale = A.scale; q.shift = A.shift; q.ovf = ctx->ovf;
    q.x_bytes = x_nchw ? (uint32_t)((unsigned long long)d->N * d->Cin * d->H * d->W * 4ull) : (uint32_t)G.xbytes;
    q.w_bytes = (uint32_t)P.w_bytes; q.Cin = d->Cin;
    q.Hq = pool ? pool_out(P.Ho, 3, 2, 1, 0) : P.Ho;
    q.Wq = pool ? pool_out(P.Wo, 3, 2, 1, 0) : P.Wo;
    const unsigned long long ybytes = (unsigned long long)d->N * q.Hq * q.Wq * (unsigned long long)d->Cout * P.ES;
    if (!in_window(ybytes)) return too_large(ctx, "pcv_conv2d_fused", "output");
    q.y_bytes = (uint32_t)ybytes;
    q.N = d->N; q.H = d->H; q.W = d->W; q.Wp = G.wpitch; q.Ho = P.Ho; q.Wo = P.Wo; q.Cout = d->Cout;
    q.kh = d->kh; q.pt = d->pad_t; q.x0off = -(d->pad_l + (d->pad_l & 1));
    q.tilesH = pool ? (q.Hq + 6) / 7 : (P.Ho + 15) / 16;
    q.tilesW = pool ? (q.Wq + 6) / 7 : (P.Wo + 15) / 16;
    const long long nT = (long long)d->N * q.tilesH * q.tilesW;
    if (nT >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_conv2d_fused: too many tiles; split the batch");
    q.nTiles = (int)nT;
    q.act = d->act;
    if (d->has_residual || d->post_act != PCV_ACT_NONE)
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: the stem kernel has no residual / post-activation path");
    const int t = d->dtype == PCV_BF16 ? 0 : 1;
    long long nb = block_slots(ctx, ctx->stem_bpc[t]);
    if (nb > nT) nb = nT;
    nb = (nb + 7) / 8 * 8;
    const bool narrow = !pool && d->Cout <= 32 && ctx->use_stem32;             // half the channel rows: stems of the MobileNet / EfficientNet families
    return launch(ctx, kStem[t][x_nchw ? 1 : 0][narrow ? STEM_NARROW : (pool ? STEM_POOLED : STEM_PLAIN)], (unsigned)nb, A.stream, q);
}

static int launch_gconv_rows(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A,
                             const GConvRPlan& gr) {
    GConvRParams q;
    std::memset(&q, 0, sizeof(q));
    q.x = A.x; q.y = A.y; q.scale = A.scale; q.shift = A.shift; q.ovf = ctx->ovf;
    q.w = static_cast<const char*>(A.packed) + P.gconv_off;
    q.x_bytes = (uint32_t)G.xbytes; q.w_bytes = (uint32_t)(P.total_bytes - P.gconv_off);
    q.y_bytes = (uint32_t)(G.M64 * (unsigned long long)d->Cin * 2ull);
    q.Min = d->N * d->H * d->W; q.Mout = (int)G.M64;
    q.W = d->W; q.Wo = P.Wo; q.Ho = P.Ho; q.C = d->Cin;
    q.R = gr.R; q.RWo = gr.R * P.Wo; q.XH = gr.XH; q.xl = gr.xl; q.win = gr.win;
    q.div_wo = make_fastdiv((uint32_t)P.Wo);
    q.div_ho = make_fastdiv((uint32_t)P.Ho);
    const long long rows = (long long)d->N * P.Ho;
    q.nRowTiles = (int)((rows + gr.R - 1) / gr.R);
    const long long nT = (long long)q.nRowTiles * (d->Cin / 64);
    if (nT >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_conv2d_fused: too many tiles; split the batch");
    q.nTiles = (int)nT;
    q.act = d->act;
    const int lds = 2 * gr.xl * 32 * 128;
    long long nb = block_slots(ctx, lds * 2 <= kGconvRMaxLds ? 2 : 1);
    if (nb > nT) nb = nT;
    nb = (nb + 7) / 8 * 8;
    return launch(ctx, gconvr_kernel(d->dtype, d->stride_h, P.gconv_kt, lds), (unsigned)nb, A.stream, q);
}

static int launch_gconvx(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A,
                         const GConvXPlan& gx) {
    GConvXParams q;
    std::memset(&q, 0, sizeof(q));
    q.x = A.x; q.y = A.y; q.scale = A.scale; q.shift = A.shift; q.ovf = ctx->ovf;
    q.w = static_cast<const char*>(A.packed) + P.gconvx_off;
    q.x_bytes = (uint32_t)G.xbytes; q.w_bytes = (uint32_t)(P.total_bytes - P.gconvx_off);
    q.y_bytes = (uint32_t)(G.M64 * (unsigned long long)d->Cin * 2ull);
    q.Min = d->N * d->H * d->W; q.Mout = (int)G.M64;
    q.W = d->W; q.Wo = P.Wo; q.Ho = P.Ho; q.C = d->Cin;
    q.G = d->groups; q.GB = gx.GB;
    q.R = gx.R; q.RWo = gx.R * P.Wo; q.npb = (q.RWo + 15) / 16; q.win = gx.win; q.pitch = gx.pitch;
    q.div_wo = make_fastdiv((uint32_t)P.Wo);
    q.div_ho = make_fastdiv((uint32_t)P.Ho);
    q.div_cpb = make_fastdiv((uint32_t)(gx.GB * (P.Cg_in / 8)));
    const long long rows = (long long)d->N * P.Ho;
    q.nRowTiles = (int)((rows + gx.R - 1) / gx.R);
    const long long nT = (long long)q.nRowTiles * ((d->groups + gx.GB - 1) / gx.GB);
    if (nT >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_conv2d_fused: too many tiles; split the batch");
    q.nTiles = (int)nT;
    q.act = d->act;
    long long nb = block_slots(ctx, ctx->gconvx_bpc[gx.pbi]);
    if (nb > nT) nb = nT;
    nb = (nb + 7) / 8 * 8;
    Kernel k = kGConvX[d->dtype == PCV_BF16 ? 0 : 1][d->stride_h - 1][gx.pbi][gconvx_width(P.Cg_in)];
    k.lds = gx.lds;
    return launch(ctx, k, (unsigned)nb, A.stream, q);
}

static int launch_gconv_flat(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A) {
    GConvParams q;
    std::memset(&q, 0, sizeof(q));
    q.x = A.x; q.y = A.y; q.scale = A.scale; q.shift = A.shift; q.ovf = ctx->ovf;
    q.w = static_cast<const char*>(A.packed) + P.gconv_off;
    q.x_bytes = (uint32_t)G.xbytes; q.w_bytes = (uint32_t)(P.total_bytes - P.gconv_off);
    q.y_bytes = (uint32_t)(G.M64 * (unsigned long long)d->Cin * 2ull);
    q.M = (int)G.M64; q.H = d->H; q.W = d->W; q.C = d->Cin; q.HW = d->H * d->W;
    q.div_hw = make_fastdiv((uint32_t)q.HW);
    q.div_w = make_fastdiv((uint32_t)d->W);
    q.nPixTiles = (int)((G.M64 + 127) / 128);
    const long long nT = (long long)q.nPixTiles * (d->Cin / 64);
    if (nT >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_conv2d_fused: too many tiles; split the batch");
    q.nTiles = (int)nT;
    q.act = d->act;
    const int slot = gconv_slot(d->W);
    long long nb = block_slots(ctx, ctx->gconv_bpc[slot]);
    if (nb > nT) nb = nT;
    nb = (nb + 7) / 8 * 8;
    return launch(ctx, gconv_kernel(d->dtype, slot), (unsigned)nb, A.stream, q);
}

// y's channel pitch in elements (y_cpitch, 0 = dense) and its extent in bytes. Y_ALIGNED: every pixel's channels start on 16 bytes;
// Y_DENSE_ANY: a dense y (pitch == Cout) may also have any channel count (the generic kernel's ragged variants)
enum YPitchRule { Y_ALIGNED, Y_DENSE_ANY };
static int y_pitch(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvGeom& G, YPitchRule rule, int* ypitch, unsigned long long* ybytes) {
    const int es = esize(d->out_dtype);
    *ypitch = d->y_cpitch > 0 ? d->y_cpitch : d->Cout;
    if (*ypitch < d->Cout || (!(rule == Y_DENSE_ANY && *ypitch == d->Cout) && (*ypitch * es) % 16 != 0))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: y_cpitch must be >= Cout and a multiple of 16 bytes");
    *ybytes = ((G.M64 - 1) * (unsigned long long)*ypitch + d->Cout) * es;
    return PCV_OK;
}

static const Kernel kNoKernel = {nullptr, 0, 0, 0, 0};
static const Kernel& d3_kernel(const ConvRoute& R, const pcv_conv_desc* d) {
    const int t = d->dtype == PCV_BF16 ? 0 : 1;
    switch (R.kernel) {
        case CK_D3C: return kD3C[0][t];
        case CK_D3K: return kD3K[0][t];
        case CK_D3I: return kD3I[d->Cin == 256 ? 0 : 1][t];
        case CK_D1I: return kD1I[d->Cin == 1024 ? 0 : 1][t];
        case CK_D3W: return kD3W[R.shape][t];
        case CK_P1R: return kP1R[R.shape][t];
        case CK_D3Q_1X1: return kD1[R.shape][t];
        case CK_D3Q: return kD3[R.shape][t];
        default: return kNoKernel;              // not a D3Params kernel
    }
}
// Every kernel that takes D3Params (CK_D3I .. CK_D3Q_1X1; all 16 bit): the dense 3x3 ones and, with the parameter block in its 1x1 mode
// (H / W / HW describe the OUTPUT map, a strided 1x1 reads every stride-th pixel), p1r / d1i / d3q's 1x1 shapes
static int launch_d3(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A, const ConvRoute& R) {
    const ConvKernel ck = R.kernel;
    const Kernel& K = d3_kernel(R, d);
    if (!K.fn) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: no kernel for this route");
    const bool one = ck == CK_P1R || ck == CK_D1I || ck == CK_D3Q_1X1;
    const bool own_blob = ck == CK_D3I || ck == CK_D1I;       // the fragment-ordered copy behind the generic blob (ConvPlan::d3i_off)
    int ypitch = 0;
    unsigned long long ybytes = 0;
    if (int rc = y_pitch(ctx, d, G, Y_ALIGNED, &ypitch, &ybytes)) return rc;
    if (!in_window(ybytes)) return too_large(ctx, "pcv_conv2d_fused", "output");
    D3Params q;
    std::memset(&q, 0, sizeof(q));
    q.x = A.x; q.res = d->has_residual ? A.residual : nullptr; q.y = A.y;
    q.w = static_cast<const char*>(A.packed) + (own_blob ? P.d3i_off : P.ktab_bytes);
    q.scale = A.scale; q.shift = A.shift; q.ovf = ctx->ovf;
    if (!own_blob) q.dbgflags = ctx->dbg_flags;
    q.x_bytes = (uint32_t)G.xbytes; q.w_bytes = (uint32_t)(own_blob ? P.total_bytes - P.d3i_off : P.w_bytes); q.y_bytes = (uint32_t)ybytes;
    q.res_bytes = (uint32_t)(G.M64 * (unsigned long long)d->Cout * 2ull);
    q.M = (int)G.M64; q.Cout = d->Cout; q.Ypitch = ypitch; q.Cin = d->Cin; q.Kpad = P.Kpad;
    q.Hin = d->H; q.Win = d->W;
    if (one) {
        q.H = P.Ho; q.W = P.Wo; q.HW = P.Ho * P.Wo;
        q.div_w = make_fastdiv((uint32_t)P.Wo);
        q.stride = d->stride_h;
        q.nk = d->Cin / 64; q.slices = q.nk;
    } else {
        q.H = d->H; q.W = d->W; q.HW = d->H * d->W;
        q.div_w = make_fastdiv((uint32_t)d->W);
        q.stride = 1;
        q.nk = P.nk; q.slices = d->Cin / 64;
    }
    // (diagnostic builds: -DD3X3_STAMPS, -DD3W_CYCLES, -DD3C_CYCLES, -DD3I_CYCLES, -DD1I_CYCLES, -DP1R_CYCLES; d3q's 1x1 shapes have none)
    if (ck != CK_D3Q_1X1) q.dbg = reinterpret_cast<uint32_t*>(ctx->dbg_ptr);
    q.div_hw = make_fastdiv((uint32_t)q.HW);
    q.act = d->act; q.post_act = d->post_act;
    q.nChTiles = (d->Cout + K.BM - 1) / K.BM;
    static_assert(D3CCfg::ROWS == D3KCfg::ROWS, "launch_d3 computes the tile count of d3c AND d3k from one ROWS constant");
    long long nT;
    switch (ck) {
        case CK_D3C:            // tiles = ROWS output rows of one image (route_conv counts with each kernel's own constant)
        case CK_D3K:
            nT = (long long)d->N * ((d->H + D3CCfg::ROWS - 1) / D3CCfg::ROWS) * q.nChTiles;
            break;
        case CK_D3I: {          // one block per (image, or two 7 x 7 images; 256-channel tile)
            const int nimg = d->Cin == 256 ? D3ICfgT<256>::NIMG : D3ICfgT<512>::NIMG;
            nT = (long long)((d->N + nimg - 1) / nimg) * q.nChTiles;
            break;
        }
        default: nT = ((long long)((G.M64 + K.BP - 1) / K.BP)) * q.nChTiles;       // (d1i: channel tiles of a pixel tile side by side)
    }
    if (nT >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_conv2d_fused: too many tiles; split the batch");
    q.nTiles = (int)nT;
    long long nb = nT;          // d3i / d1i: one block per tile
    if (!own_blob) {            // the others: a persistent grid of one block per CU, a multiple of 8 so that every XCD gets the same number
        const long long slots = block_slots(ctx, 1);
        nb = slots < nT ? slots : nT;
        nb = (nb + 7) / 8 * 8;
    }
    if (ck == CK_P1R && nT > nb) {
        // p1r: equal tiles on a persistent grid leave the last round partly empty (12.25 rounds = 13). When the remainder splits evenly -
        // its tiles into 16-pixel units, one per block, every block getting a unit of its own channel group - the kernel runs it as
        // one-unit pseudo tiles behind the full rounds (p1r_conv.hpp, `tailN`).
        const long long nCG = q.nChTiles, TP = K.BP / 16, rem = nT % nb;
        if (rem > 0 && nb % (8 * nCG) == 0 && rem % nCG == 0 && rem * TP <= nb && ctx->use_p1r != 3 && ctx->use_p1r != -3) {        // ("p1r" = 3 / -3: forced / automatic routing without the split tail, for A/B)
            q.nTiles = (int)(nT - rem);
            q.tailN = (int)rem;
        }
    }
    return launch(ctx, K, (unsigned)nb, A.stream, q);
}

// dense layer on a 1x1 map, fp32 (classifier): many small blocks instead of a handful of 128x128 tiles
static int launch_head(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A) {
    const int ypitch = d->y_cpitch > 0 ? d->y_cpitch : d->Cout;
    if (ypitch < d->Cout) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: y_cpitch must be >= Cout");
    HeadParams q;
    q.x = static_cast<const float*>(A.x); q.w = reinterpret_cast<const float*>(static_cast<const char*>(A.packed) + P.ktab_bytes);
    q.scale = A.scale; q.shift = A.shift; q.y = static_cast<float*>(A.y);
    q.M = d->N; q.K = d->Cin; q.Kpad = P.Kpad; q.Cout = d->Cout; q.Xpitch = G.cpitch; q.Ypitch = ypitch; q.act = d->act;
    const unsigned gx = (unsigned)(P.wrows / 32);
    const bool wide = (long long)gx * ((d->N + 31) / 32) >= 2ll * ctx->num_cu;      // enough 32-image blocks for two per CU
    if (wide) hipLaunchKernelGGL(head_gemm_f32_kernel<32>, dim3(gx, (unsigned)((d->N + 31) / 32)), dim3(256), 0, A.stream, q);
    else hipLaunchKernelGGL(head_gemm_f32_kernel<16>, dim3(gx, (unsigned)((d->N + 15) / 16)), dim3(256), 0, A.stream, q);
    return launched(ctx);
}

static int launch_igemm(pcv_ctx* ctx, const pcv_conv_desc* d, const ConvPlan& P, const ConvGeom& G, const ConvArgs& A, const ConvRoute& R) {
    if (R.special && P.ngb != 1 && ((d->Cout % 8 != 0) || (P.cout_blk % 8 != 0)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: ragged channel count with groups unsupported");
    const int tile = R.tile, khw = R.khw;
    const Kernel T = igemm_kernel(d->dtype, d->out_dtype, R.special, tile, khw);
    if (!T.fn) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: no kernel for this dtype combination");

    IgemmParams p;
    p.x = A.x;
    p.ktab = reinterpret_cast<const uint32_t*>(A.packed);
    p.w = static_cast<const char*>(A.packed) + P.ktab_bytes;
    p.res = d->has_residual ? A.residual : nullptr;
    p.gate = A.gate;
    p.ovf = ctx->ovf;
    p.y = A.y;
    p.scale = A.scale;
    p.shift = A.shift;
    p.x_bytes = (uint32_t)G.xbytes;
    p.w_bytes = (uint32_t)P.w_bytes;
    int ypitch = 0;
    unsigned long long ybytes = 0;
    if (int rc = y_pitch(ctx, d, G, Y_DENSE_ANY, &ypitch, &ybytes)) return rc;
    if (!in_window(ybytes) && d->out_dtype != PCV_F32) return too_large(ctx, "pcv_conv2d_fused", "output");
    p.y_bytes = ybytes >= 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)ybytes;
    p.M = (int)G.M64;
    p.Cout = P.cout_blk;
    p.Cout_total = d->Cout;
    p.Ypitch = ypitch;
    p.cout_blk = P.cout_blk;
    p.cin_blk = d->groups == 1 ? 0 : P.cin_blk;
    p.wrows_blk = P.wrows;
    p.HoWo = P.Ho * P.Wo;
    p.Wo = P.Wo;
    p.div_howo = make_fastdiv((uint32_t)p.HoWo);
    p.div_wo = make_fastdiv((uint32_t)p.Wo);
    p.H = d->H;
    p.W = d->W;
    p.Wpitch = G.wpitch;
    p.Cpitch = G.cpitch;
    p.sh = d->stride_h;
    p.sw = d->stride_w;
    p.pt = d->pad_t;
    p.pl = d->pad_l;
    p.nR = P.nR;
    p.nQ = P.nQ;
    for (int i = 0; i < IGEMM_MAX_TAPS; ++i) { p.dy[i] = P.dy[i]; p.dx[i] = P.dx[i]; }
    p.nk = P.nk;
    p.Kpad = P.Kpad;
    p.act = d->act;
    p.post_act = d->post_act;
    p.nPixTiles = (p.M + T.BP - 1) / T.BP;
    p.nChTiles = (P.cout_blk + T.BM - 1) / T.BM;
    p.ngb = P.ngb;
    p.Cin = P.cin_blk;
    p.ksteps_per_tap = P.cin_blk / (8 * P.CE) > 0 ? P.cin_blk / (8 * P.CE) : 1;
    p.korder = P.conv3 ? 1 : 0;
    const long long nTiles = (long long)p.nPixTiles * p.nChTiles * P.ngb;
    if (nTiles >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_conv2d_fused: too many tiles; split the batch");
    p.nTiles = (int)nTiles;
    // persistent grid: what is resident at once, a multiple of 8 so that every XCD gets the same number of blocks
    const int bpc = R.special ? ctx->igemm_bpc[d->dtype][1][tile][0] : ctx->igemm_bpc[d->dtype][0][tile][khw_slot(khw)];
    // Short K loops (HBM-bound 1x1 layers) run persistent, so that the next tile's loads overlap this tile's
    // epilogue; long K loops run one tile per block (the dispatcher refills a CU while the finished block's stores drain).
    const bool persistent = ctx->persist_mode == 1 || (ctx->persist_mode < 0 && P.nk <= ctx->persist_max_nk);
    long long nblocks = persistent ? block_slots(ctx, bpc) : nTiles;
    if (nblocks > nTiles) nblocks = nTiles;
    nblocks = (nblocks + 7) / 8 * 8;
    p.wstat = (ctx->use_wstat && persistent && P.nk == 1 && p.nChTiles == 1 && P.ngb == 1) ? 1 : 0;
    return launch(ctx, T, (unsigned)nblocks, A.stream, p);
}

static int conv2d_impl(pcv_ctx* ctx, const pcv_conv_desc* d, const void* x, const void* packed, const float* scale,
                       const float* shift, const void* residual, void* y, void* stream, bool pool, const float* gate = nullptr,
                       bool x_nchw = false) {
    PCV_ENTER(ctx);
    if (!d || !x || !packed || !y) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: NULL argument");
    if (d->has_residual && !residual) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: has_residual but residual is NULL");
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: empty input");
    if (d->groups > 1 && d->groups == d->Cin && d->Cin == d->Cout)
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: depthwise convolution goes through pcv_dwconv2d_fused");
    ConvPlan P;
    const char* why = plan_conv(*d, P, false);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_conv2d_fused: ") + why);
    if (P.Ho <= 0 || P.Wo <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: empty output");
    ConvGeom G;
    G.cpitch = d->x_cpitch > 0 ? d->x_cpitch : d->Cin;
    G.wpitch = d->x_wpitch > 0 ? d->x_wpitch : d->W;
    G.xbytes = (unsigned long long)d->N * d->H * G.wpitch * G.cpitch * P.ES;
    G.M64 = (unsigned long long)d->N * P.Ho * P.Wo;
    G.sliced_y = d->y_cpitch > 0 && d->y_cpitch != d->Cout;
    if (!in_window(G.xbytes) || G.M64 >= 0x7FFFFFFFull) return too_large(ctx, "pcv_conv2d_fused", "input");
    if (!aligned16(x) || !aligned16(packed) || !aligned16(y) || (residual && !aligned16(residual)) ||
        (scale && !aligned16(scale)) || (shift && !aligned16(shift)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: pointers must be 16-byte aligned");
    if (P.stem && G.sliced_y) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_fused: the stem kernel writes a dense y only");
    if (gate && (P.stem || pool)) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_gated_fused: the stem kernel has no gate");
    if (pool && !P.stem) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_maxpool_fused: only the stem convolution has a fused max-pool");
    if (x_nchw && (!P.stem || d->Cin > 3 || d->W % 4 != 0))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_nchw_stem_fused: only the stem convolution (<= 3 input planes, W a multiple of 4)");
    if (x_nchw && !in_window((unsigned long long)d->N * d->Cin * d->H * d->W * 4ull))
        return too_large(ctx, "pcv_conv2d_nchw_stem_fused", "the fp32 image batch");

    const ConvArgs A{x, packed, scale, shift, residual, y, gate, (hipStream_t)stream, pool, x_nchw};
    const ConvRoute R = route_conv(ctx, d, P, G, A);
    switch (R.kernel) {
        case CK_STEM: return launch_stem(ctx, d, P, G, A);
        case CK_GCONV_ROWS: return launch_gconv_rows(ctx, d, P, G, A, R.rows);
        case CK_GCONV_FLAT: return launch_gconv_flat(ctx, d, P, G, A);
        case CK_GCONVX: return launch_gconvx(ctx, d, P, G, A, R.xrows);
        case CK_D3I: case CK_D1I: case CK_D3K: case CK_D3C: case CK_D3W: case CK_D3Q: case CK_P1R: case CK_D3Q_1X1:
            return launch_d3(ctx, d, P, G, A, R);                      // the kernels that take D3Params
        case CK_HEAD: return launch_head(ctx, d, P, G, A);
        default: return launch_igemm(ctx, d, P, G, A, R);
    }
}

int pcv_conv2d_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const void* x, const void* packed, const float* scale,
                     const float* shift, const void* residual, void* y, void* stream) {
    return conv2d_impl(ctx, d, x, packed, scale, shift, residual, y, stream, false);
}

int pcv_conv2d_gated_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const void* x, const void* packed, const float* scale,
                           const float* shift, const float* gate, const void* residual, void* y, void* stream) {
    if (!ctx) return PCV_ERR_INVALID;
    if (!gate || !aligned16(gate)) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_gated_fused: gate must be a 16-byte aligned [N][Cout] fp32 array");
    if (d && d->Cout % 4 != 0) return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_gated_fused: Cout must be a multiple of 4");
    return conv2d_impl(ctx, d, x, packed, scale, shift, residual, y, stream, false, gate);
}

int pcv_fc_f32(pcv_ctx* ctx, const float* in, const float* w, const float* b, float* out, int N, int K, int J, int act,
               void* stream) {
    PCV_ENTER(ctx);
    if (!in || !w || !b || !out || N <= 0 || K <= 0 || J <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_fc_f32: bad argument");
    launch_se_fc(in, w, b, out, N, K, J, act, (hipStream_t)stream);
    return launched(ctx);
}

int pcv_gconvx_supported(const pcv_conv_desc* d) {
    if (!d) { fail(nullptr, PCV_ERR_INVALID, "pcv_gconvx_supported: NULL argument"); return 0; }
    ConvPlan P;
    const char* why = plan_conv(*d, P, false);
    if (!why && (d->N <= 0 || d->H <= 0 || d->W <= 0 || P.Ho <= 0 || P.Wo <= 0)) why = "empty input or output";
    if (!why) {
        ConvGeom G;
        G.cpitch = d->x_cpitch > 0 ? d->x_cpitch : d->Cin;
        G.wpitch = d->x_wpitch > 0 ? d->x_wpitch : d->W;
        G.xbytes = (unsigned long long)d->N * d->H * G.wpitch * G.cpitch * P.ES;
        G.M64 = (unsigned long long)d->N * P.Ho * P.Wo;
        G.sliced_y = d->y_cpitch > 0 && d->y_cpitch != d->Cout;
        why = gconvx_launch_why(*d, P, G, false, nullptr);
    }
    if (why) { fail(nullptr, PCV_ERR_INVALID, std::string("pcv_gconvx_supported: ") + why); return 0; }
    return 1;
}

int pcv_conv2d_maxpool_supported(const pcv_conv_desc* d, int k, int s, int p, int ceil_mode) {
    if (!d || k != 3 || s != 2 || p != 1 || ceil_mode) return 0;
    ConvPlan P;
    if (plan_conv(*d, P, false) != nullptr || !P.stem) return 0;
    if (d->act != PCV_ACT_RELU && d->act != PCV_ACT_RELU6) return 0;     // the kernel pools packed non-negative 16-bit values
    return (d->has_residual || d->post_act != PCV_ACT_NONE || (d->y_cpitch > 0 && d->y_cpitch != d->Cout)) ? 0 : 1;
}

int pcv_conv2d_maxpool_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const void* x, const void* packed, const float* scale,
                             const float* shift, void* y, int k, int s, int p, int ceil_mode, void* stream) {
    if (!ctx) return PCV_ERR_INVALID;
    if (!pcv_conv2d_maxpool_supported(d, k, s, p, ceil_mode))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_maxpool_fused: only the stem convolution followed by MaxPool2d(3, 2, 1) is covered");
    return conv2d_impl(ctx, d, x, packed, scale, shift, nullptr, y, stream, true);
}

int pcv_conv2d_nchw_stem_supported(const pcv_conv_desc* d, int pool) {
    if (!d) return 0;
    ConvPlan P;
    if (plan_conv(*d, P, false) != nullptr || !P.stem || d->Cin > 3 || d->W % 4 != 0) return 0;
    if (d->has_residual || d->post_act != PCV_ACT_NONE || (d->y_cpitch > 0 && d->y_cpitch != d->Cout)) return 0;
    return (!pool || pcv_conv2d_maxpool_supported(d, 3, 2, 1, 0)) ? 1 : 0;
}

int pcv_conv2d_nchw_stem_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const float* x_nchw, const void* packed, const float* scale,
                               const float* shift, void* y, int pool, void* stream) {
    if (!ctx) return PCV_ERR_INVALID;
    if (!pcv_conv2d_nchw_stem_supported(d, pool))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv2d_nchw_stem_fused: only the stride-2 stem convolution (<= 3 planes, W % 4 == 0, <= 64 channels) is covered");
    return conv2d_impl(ctx, d, x_nchw, packed, scale, shift, nullptr, y, stream, pool != 0, nullptr, true);
}

// Rows per thread of the depthwise launches (`cols` columns of channel chunks, Ho output rows): the whole column when that still
// fills the chip (>= ~16 waves per CU), else shorter strips of at least 4 rows; the dw_th tuning overrides the choice.
static void dw_strips(const pcv_ctx* ctx, int Ho, long cols, int* TH_out, int* nseg_out) {
    const long want = (long)ctx->num_cu * 64 * 16;
    int nseg = (int)((want + cols - 1) / cols);
    if (nseg < 1) nseg = 1;
    int TH = (Ho + nseg - 1) / nseg;
    if (TH < 4) TH = Ho < 4 ? Ho : 4;
    if (ctx->dw_th > 0) TH = ctx->dw_th < Ho ? ctx->dw_th : Ho;
    *TH_out = TH;
    *nseg_out = (Ho + TH - 1) / TH;
}

int pcv_dwconv2d_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const void* x, const void* packed, const float* scale,
                       const float* shift, const void* residual, void* y, void* stream) {
    PCV_ENTER(ctx);
    if (!d || !x || !packed || !y || !scale || !shift) return fail(ctx, PCV_ERR_INVALID, "pcv_dwconv2d_fused: NULL argument");
    const char* why = check_dw(*d);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_dwconv2d_fused: ") + why);
    if (d->has_residual && !residual) return fail(ctx, PCV_ERR_INVALID, "pcv_dwconv2d_fused: has_residual but residual is NULL");
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_dwconv2d_fused: empty input");
    if (!aligned16(x) || !aligned16(packed) || !aligned16(y) || !aligned16(scale) || !aligned16(shift) ||
        (residual && !aligned16(residual)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_dwconv2d_fused: pointers must be 16-byte aligned");
    DwParams p;
    p.x = x;
    p.w = packed;
    p.res = d->has_residual ? residual : nullptr;
    p.y = y;
    p.scale = scale;
    p.shift = shift;
    p.ovf = ctx->ovf;
    p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->Cin;
    const unsigned long long xbytes = (unsigned long long)d->N * d->H * d->W * d->Cin * esize(d->dtype);
    if (!in_window(xbytes)) return too_large(ctx, "pcv_dwconv2d_fused", "input");
    p.x_bytes = (uint32_t)xbytes;
    p.Ho = (d->H + d->pad_t + d->pad_b - (d->kh - 1) - 1) / d->stride_h + 1;
    p.Wo = (d->W + d->pad_l + d->pad_r - (d->kw - 1) - 1) / d->stride_w + 1;
    if (p.Ho <= 0 || p.Wo <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_dwconv2d_fused: empty output");
    p.pt = d->pad_t; p.pl = d->pad_l;
    p.C8 = d->Cin / (d->kh == 5 ? 4 : 8);          // channel chunks per pixel (5x5 runs 4 channels per thread)
    const long cols = (long)d->N * p.Wo * p.C8;
    dw_strips(ctx, p.Ho, cols, &p.TH, &p.nseg);
    p.act = d->act;
    p.post_act = d->post_act;
    p.total = cols * p.nseg;
    p.flags = ctx->dw_flags;
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_dwconv2d_fused", p.total, &grid)) return rc;
    const Kernel& K = kDw[dt_index(d->dtype)][(d->kh == 3 ? 0 : 2) + d->stride_h - 1][d->act <= PCV_ACT_RELU6 && d->post_act <= PCV_ACT_RELU6 ? 1 : 0];
    return launch(ctx, K, grid, (hipStream_t)stream, p);
}

// ---- depthwise MixConv (mixconv.hpp) ---------------------------------------------------------------------------------------------
// every argument check of the three entry points; G = nk on success
static const char* check_mix(const pcv_conv_desc& d, const int* ks, int nk, MixPlan& P) {
    if (desc_stale(d)) return kStaleDesc;
    if (!dtype_ok(d.dtype) || d.out_dtype != d.dtype) return "mixconv: out_dtype must equal dtype";
    if (d.groups != d.Cin || d.Cin != d.Cout) return "mixconv: needs groups == Cin == Cout (the 1x1 MixConv is pcv_conv2d_fused with groups = 2)";
    if (!ks || nk < 2 || nk > kMixMaxGroups) return "mixconv: the kernel list must be 3, 5, ..., 3 + 2 (G - 1) with G = 2 .. 5";
    for (int g = 0; g < nk; ++g)
        if (ks[g] != 3 + 2 * g) return "mixconv: the kernel list must be 3, 5, ..., 3 + 2 (G - 1) with G = 2 .. 5";
    if (d.kh != ks[nk - 1] || d.kw != ks[nk - 1]) return "mixconv: kh / kw must be the largest window of the list";
    if (d.pad_t != d.kh / 2 || d.pad_b != d.kh / 2 || d.pad_l != d.kh / 2 || d.pad_r != d.kh / 2)
        return "mixconv: padding must be k / 2 of every window (pad fields: that of the largest)";
    if (d.stride_h != d.stride_w || (d.stride_h != 1 && d.stride_h != 2)) return "mixconv: stride 1 or 2";
    if (d.dil_h != 1 || d.dil_w != 1) return "mixconv: dilation unsupported";
    if (d.has_residual || d.post_act != PCV_ACT_NONE) return "mixconv: no residual / post-activation (MixUnit has none behind conv1)";
    if (d.act < PCV_ACT_NONE || d.act > PCV_ACT_HSWISH) return "mixconv: unknown activation";
    if (d.x_cpitch > 0 && d.x_cpitch != d.Cin) return "mixconv: padded channel pitch unsupported";
    if (d.x_wpitch > 0 && d.x_wpitch != d.W) return "mixconv: padded row pitch unsupported";
    if (d.y_cpitch > 0 && d.y_cpitch != d.Cout) return "mixconv: y must be dense";
    const char* why = nullptr;
    if (!mix_plan(d.Cin, nk, esize(d.dtype), P, &why)) return why;
    return nullptr;
}

int pcv_mixconv_packed_bytes(const pcv_conv_desc* d, const int* kernels, int nk, size_t* bytes) {
    MixPlan P;
    if (!d || !bytes) return fail(nullptr, PCV_ERR_INVALID, "pcv_mixconv_packed_bytes: NULL argument");
    if (const char* why = check_mix(*d, kernels, nk, P)) return fail(nullptr, PCV_ERR_INVALID, std::string("pcv_mixconv_packed_bytes: ") + why);
    *bytes = P.bytes;
    return PCV_OK;
}

int pcv_mixconv_pack(pcv_ctx* ctx, const pcv_conv_desc* d, const int* kernels, int nk, const float* const* w, void* packed, void* stream) {
    PCV_ENTER(ctx);
    if (!d || !w || !packed) return fail(ctx, PCV_ERR_INVALID, "pcv_mixconv_pack: NULL argument");
    MixPlan P;
    if (const char* why = check_mix(*d, kernels, nk, P)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_mixconv_pack: ") + why);
    if (!aligned16(packed)) return fail(ctx, PCV_ERR_INVALID, "pcv_mixconv_pack: packed buffer must be 16-byte aligned");
    MixPackParams q = {};
    q.out = packed;
    q.G = nk;
    q.wr = d->Cin / nk;
    q.w0 = d->Cin - (nk - 1) * q.wr;
    long long total = 0;
    for (int g = 0; g < kMixMaxGroups; ++g) {
        if (g < nk && !w[g]) return fail(ctx, PCV_ERR_INVALID, "pcv_mixconv_pack: NULL weight pointer in the list");
        q.w[g] = g < nk ? w[g] : nullptr;
        q.cbeg[g] = P.cbeg[g];
        q.span[g] = P.span[g];
        q.woff[g] = P.woff[g];
        total += (long long)(3 + 2 * g) * (3 + 2 * g) * P.span[g];
        q.elem_end[g] = (int)total;
    }
    if (total >= 0x7fffffffll) return too_large(ctx, "pcv_mixconv_pack", "the blob");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_mixconv_pack", total, &grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    for_dtype(d->dtype, [&](auto T) { pack_mix_kernel<DT_OF(T)><<<grid, 256, 0, s>>>(q); });
    return launched(ctx);
}

int pcv_mixconv2d_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const int* kernels, int nk, const void* x, const void* packed,
                        const float* scale, const float* shift, void* y, void* stream) {
    PCV_ENTER(ctx);
    if (!d || !x || !packed || !y || !scale || !shift) return fail(ctx, PCV_ERR_INVALID, "pcv_mixconv2d_fused: NULL argument");
    MixPlan P;
    if (const char* why = check_mix(*d, kernels, nk, P)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_mixconv2d_fused: ") + why);
    if (d->N <= 0 || d->H <= 0 || d->W <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_mixconv2d_fused: empty input");
    if (!aligned16(x) || !aligned16(packed) || !aligned16(y) || !aligned16(scale) || !aligned16(shift))
        return fail(ctx, PCV_ERR_INVALID, "pcv_mixconv2d_fused: pointers must be 16-byte aligned");
    MixParams p = {};
    p.x = x;
    p.w = packed;
    p.y = y;
    p.scale = scale;
    p.shift = shift;
    p.ovf = ctx->ovf;
    p.N = d->N; p.H = d->H; p.W = d->W; p.C = d->Cin;
    const unsigned long long xbytes = (unsigned long long)d->N * d->H * d->W * d->Cin * esize(d->dtype);
    if (!in_window(xbytes)) return too_large(ctx, "pcv_mixconv2d_fused", "input");
    p.x_bytes = (uint32_t)xbytes;
    p.Ho = (d->H - 1) / d->stride_h + 1;           // pad k / 2 on both sides: the same for every window of the list
    p.Wo = (d->W - 1) / d->stride_w + 1;
    dw_strips(ctx, p.Ho, (long)d->N * p.Wo * (d->Cin / 4), &p.TH, &p.nseg);          // (columns of 4-channel chunks)
    p.act = d->act;
    p.flags = ctx->dw_flags;
    long long blocks = 0;
    for (int g = 0; g < kMixMaxGroups; ++g) {
        p.cbeg[g] = P.cbeg[g];
        p.span[g] = P.span[g];
        p.nchunk[g] = P.span[g] / P.cpt[g];
        p.woff[g] = P.woff[g];
        unsigned nb = 0;
        if (int rc = flat_grid(ctx, "pcv_mixconv2d_fused", (long long)d->N * p.nseg * p.Wo * p.nchunk[g], &nb)) return rc;
        blocks += nb;
        if (blocks > 0x7fffffffll) return too_large(ctx, "pcv_mixconv2d_fused", "the grid");
        p.blk_end[g] = (uint32_t)blocks;
    }
    const Kernel& K = kMix[dt_index(d->dtype)][d->stride_h - 1][d->act <= PCV_ACT_RELU6 ? 1 : 0][nk - 2];
    return launch(ctx, K, (unsigned)blocks, (hipStream_t)stream, p);
}

// ---- ghost module: cheap depthwise 3x3 + concatenation + skip add (ghost.hpp) ------------------------------------------------------
// every check of the descriptor alone (the pointer checks are the launch's)
static const char* check_ghost(const pcv_conv_desc& d) {
    if (desc_stale(d)) return kStaleDesc;
    if (!dtype_ok(d.dtype) || d.out_dtype != d.dtype) return "ghost: out_dtype must equal dtype";
    constexpr int kMaxChannels = 1 << 20, kMaxExtent = 1 << 24;
    if (d.Cin <= 0 || d.Cin > kMaxChannels) return "ghost: channel count out of range (1 .. 2^20)";
    if (d.groups != d.Cin || d.Cin != d.Cout) return "ghost: needs groups == Cin == Cout (the cheap convolution is depthwise)";
    if (d.Cin % 4 != 0) return "ghost: the half width Cm must be a multiple of 4 channels";
    if (d.kh != 3 || d.kw != 3) return "ghost: the cheap convolution's window must be 3x3";
    if (d.stride_h != 1 || d.stride_w != 1) return "ghost: stride must be 1";
    if (d.pad_t != 1 || d.pad_b != 1 || d.pad_l != 1 || d.pad_r != 1) return "ghost: padding must be 1 on every side";
    if (d.dil_h != 1 || d.dil_w != 1) return "ghost: dilation unsupported";
    if (d.post_act != PCV_ACT_NONE) return "ghost: post_act unsupported (nothing follows the skip add of GhostUnit)";
    if (d.act < PCV_ACT_NONE || d.act > PCV_ACT_CLAMP01) return "ghost: unknown activation";
    if (d.x_cpitch != round_up(d.Cin, 8)) return "ghost: x_cpitch must be Cm rounded up to a multiple of 8";
    if (d.x_wpitch > 0 && d.x_wpitch != d.W) return "ghost: padded row pitch unsupported";
    if (d.y_cpitch != 0 && d.y_cpitch != 2 * d.Cin) return "ghost: y_cpitch must be 0 or 2 Cm (y is dense)";
    if (d.N > kMaxExtent || d.H > kMaxExtent || d.W > kMaxExtent) return "ghost: N / H / W out of range (> 2^24)";
    if (d.N <= 0 || d.H <= 0 || d.W <= 0) return "ghost: empty input";
    return nullptr;
}

int pcv_ghost_supported(const pcv_conv_desc* d) {
    if (!d) { fail(nullptr, PCV_ERR_INVALID, "pcv_ghost_supported: NULL argument"); return 0; }
    if (const char* why = check_ghost(*d)) { fail(nullptr, PCV_ERR_INVALID, std::string("pcv_ghost_supported: ") + why); return 0; }
    return 1;
}

int pcv_ghost_dw_fused(pcv_ctx* ctx, const pcv_conv_desc* d, const void* m, const void* packed, const float* scale,
                       const float* shift, const void* residual, void* y, void* stream) {
    PCV_ENTER(ctx);
    if (!d || !m || !packed || !y || !scale || !shift) return fail(ctx, PCV_ERR_INVALID, "pcv_ghost_dw_fused: NULL argument");
    if (const char* why = check_ghost(*d)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_ghost_dw_fused: ") + why);
    if (d->has_residual && !residual) return fail(ctx, PCV_ERR_INVALID, "pcv_ghost_dw_fused: has_residual but residual is NULL");
    if (!aligned16(m) || !aligned16(packed) || !aligned16(y) || !aligned16(scale) || !aligned16(shift) ||
        (d->has_residual && !aligned16(residual)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_ghost_dw_fused: pointers must be 16-byte aligned");
    GhostParams p = {};
    p.m = m;
    p.w = packed;
    p.res = d->has_residual ? residual : nullptr;
    p.y = y;
    p.scale = scale;
    p.shift = shift;
    p.ovf = ctx->ovf;
    p.N = d->N; p.H = d->H; p.W = d->W;
    p.Cm = d->Cin;
    p.CP = d->x_cpitch;
    p.C4 = d->Cin / 4;
    // (factor by factor: N, H, W <= 2^24 and CP <= 2^20 each, their product does not fit 64 bits)
    unsigned long long xbytes = (unsigned long long)d->N * d->H;
    if (in_window(xbytes)) xbytes *= (unsigned long long)d->W;
    if (in_window(xbytes)) xbytes *= (unsigned long long)p.CP * esize(d->dtype);
    if (!in_window(xbytes)) return too_large(ctx, "pcv_ghost_dw_fused", "input");
    p.x_bytes = (uint32_t)xbytes;
    const long cols = (long)d->N * p.W * p.C4;
    dw_strips(ctx, p.H, cols, &p.TH, &p.nseg);
    p.act = d->act;
    p.total = cols * p.nseg;
    p.flags = ctx->dw_flags;
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_ghost_dw_fused", p.total, &grid)) return rc;
    const Kernel& K = kGhost[dt_index(d->dtype)][d->act <= PCV_ACT_RELU6 ? 1 : 0];
    return launch(ctx, K, grid, (hipStream_t)stream, p);
}

static int pool_out(int in, int k, int s, int p, int ceil_mode) {
    const int num = in + 2 * p - k + (ceil_mode ? s - 1 : 0);
    if (num < 0) return 0;                                // torch divides rounding DOWN: empty (C's `/` would round -1 / 2 up to one row)
    int o = num / s + 1;
    if (ceil_mode && (o - 1) * s >= in + p) --o;          // the last window must start inside the input or the left padding
    return o;
}

int pcv_maxpool2d(pcv_ctx* ctx, const void* x, void* y, int N, int H, int W, int C, int k, int s, int p, int ceil_mode,
                  int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || s <= 0 || p < 0 || !dtype_ok(dtype) || C % 8 != 0 ||
        2 * p > k)
        return fail(ctx, PCV_ERR_INVALID, "pcv_maxpool2d: bad argument (C must be a multiple of 8, pad <= k/2)");
    const int Ho = pool_out(H, k, s, p, ceil_mode), Wo = pool_out(W, k, s, p, ceil_mode);
    if (Ho <= 0 || Wo <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_maxpool2d: empty output");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_maxpool2d", (long long)N * Ho * Wo * (C / 8), &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { maxpool_kernel<DT_OF(T)><<<grid, 256, 0, st>>>(x, y, N, H, W, C, Ho, Wo, k, s, p); });
    return launched(ctx);
}

int pcv_avgpool2d(pcv_ctx* ctx, const void* x, void* y, int N, int H, int W, int C, int k, int s, int dtype,
                  int out_dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || k <= 0 || s <= 0 || !dtype_ok(dtype) || C % 8 != 0 ||
        (out_dtype != dtype && out_dtype != PCV_F32) || k > H || k > W)
        return fail(ctx, PCV_ERR_INVALID, "pcv_avgpool2d: bad argument (C must be a multiple of 8, k <= H,W)");
    hipStream_t st = (hipStream_t)stream;
    const int Ho = (H - k) / s + 1, Wo = (W - k) / s + 1;
    if (k != H || k != W) return launch_avg(ctx, "pcv_avgpool2d", x, y, N, H, W, C, Ho, Wo, k, s, dtype, out_dtype, st);
    launch_mean(x, y, N, H * W, C, dtype, out_dtype, st);
    return launched(ctx);
}

int pcv_global_avgpool(pcv_ctx* ctx, const void* x, void* y, int N, int HW, int C, int dtype, int out_dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || N <= 0 || HW <= 0 || C <= 0 || C % 8 != 0 || !dtype_ok(dtype) ||
        (out_dtype != dtype && out_dtype != PCV_F32))
        return fail(ctx, PCV_ERR_INVALID, "pcv_global_avgpool: bad argument (C must be a multiple of 8)");
    launch_mean(x, y, N, HW, C, dtype, out_dtype, (hipStream_t)stream);
    return launched(ctx);
}

int pcv_gemm_bias(pcv_ctx* ctx, const void* x, const void* packed, const float* bias, void* y, int N, int Cin,
                  int Cout, int dtype, int out_dtype, void* stream) {
    PCV_ENTER(ctx);
    pcv_conv_desc d;
    std::memset(&d, 0, sizeof(d));
    d.struct_size = (int32_t)sizeof(d);
    d.N = N; d.H = 1; d.W = 1; d.Cin = Cin; d.Cout = Cout; d.kh = 1; d.kw = 1;
    d.stride_h = d.stride_w = 1; d.dil_h = d.dil_w = 1; d.groups = 1;
    d.act = PCV_ACT_NONE; d.post_act = PCV_ACT_NONE; d.has_residual = 0;
    d.dtype = dtype; d.out_dtype = out_dtype; d.x_cpitch = Cin; d.x_wpitch = 1;
    return pcv_conv2d_fused(ctx, &d, x, packed, nullptr, bias, nullptr, y, stream);
}

int pcv_se_squeeze(pcv_ctx* ctx, const void* x, float* mean, int N, int HW, int C, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !mean || N <= 0 || HW <= 0 || C <= 0 || C % 8 != 0 || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_se_squeeze: bad argument (C must be a multiple of 8)");
    launch_mean(x, mean, N, HW, C, dtype, PCV_F32, (hipStream_t)stream);
    return launched(ctx);
}

static void launch_se_fc(const float* in, const float* w, const float* b, float* out, int N, int K, int J, int act,
                         hipStream_t st) {
    int TJ = K >= 512 ? 32 : K >= 128 ? 64 : 256;               // long rows: split K over more threads of the block
    // (half these sizes are 1-2 % faster on the SE nets, but the different fp32 summation order moved MobileNetV3-large's bf16
    // logits from just under to just over the 1e-2 parity bound against the oracle: not worth the margin)
    while (TJ > 8 && TJ / 2 >= J) TJ /= 2;                      // few output rows: do not leave row slots idle
    dim3 grid((unsigned)((N + 7) / 8), (unsigned)((J + TJ - 1) / TJ));
    se_fc_kernel<<<grid, 256, 0, st>>>(in, w, b, out, N, K, J, TJ, act);
}

int pcv_se_excite(pcv_ctx* ctx, const float* mean, const float* w1, const float* b1, const float* w2, const float* b2,
                  float* mid, float* gate, int N, int C, int M, int mid_act, int out_act, void* stream) {
    PCV_ENTER(ctx);
    if (!mean || !w1 || !b1 || !w2 || !b2 || !mid || !gate || N <= 0 || C <= 0 || M <= 0)
        return fail(ctx, PCV_ERR_INVALID, "pcv_se_excite: bad argument");
    hipStream_t st = (hipStream_t)stream;
    launch_se_fc(mean, w1, b1, mid, N, C, M, mid_act, st);
    launch_se_fc(mid, w2, b2, gate, N, M, C, out_act, st);
    return launched(ctx);
}

int pcv_se_scale(pcv_ctx* ctx, const void* x, const float* gate, const void* residual, void* y, int N, int HW, int C,
                 int post_act, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !gate || !y || N <= 0 || HW <= 0 || C <= 0 || C % 8 != 0 || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_se_scale: bad argument (C must be a multiple of 8)");
    const long total8 = (long)N * HW * (C / 8);
    unsigned blocks = 0;
    if (int rc = stream_grid(ctx, "pcv_se_scale", total8, &blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { se_scale_kernel<DT_OF(T)><<<blocks, 256, 0, st>>>(x, gate, residual, y, total8, HW, C, post_act, ctx->ovf); });
    return launched(ctx);
}

// ---- split attention (att.py:172-189, sknet.py:59-83) and the padded average pool (resnesta.py:45-48,138-142) ---------------
int pcv_splat_squeeze(pcv_ctx* ctx, const void* x, float* s, int N, int HW, int C, int radix, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !s || N <= 0 || HW <= 0 || C <= 0 || C % 8 != 0 || radix < 1 || radix > 4 || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_splat_squeeze: bad argument (C must be a multiple of 8, radix in [1, 4])");
    launch_mean(x, s, N, HW, C, dtype, PCV_F32, (hipStream_t)stream, radix);
    return launched(ctx);
}

int pcv_splat_excite(pcv_ctx* ctx, const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* mid,
                     float* logits, float* att, int N, int C, int M, int radix, int groups, void* stream) {
    PCV_ENTER(ctx);
    if (!s || !w1 || !b1 || !w2 || !b2 || !mid || !logits || !att || N <= 0 || C <= 0 || C % 8 != 0 || M <= 0 || radix < 1 ||
        radix > 4 || groups < 1 || C % groups != 0)
        return fail(ctx, PCV_ERR_INVALID, "pcv_splat_excite: bad argument (C must be a multiple of 8 and of groups, radix in [1, 4])");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_splat_excite", (long long)N * C, &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    launch_se_fc(s, w1, b1, mid, N, C, M, PCV_ACT_RELU, st);
    launch_se_fc(mid, w2, b2, logits, N, M, radix * C, PCV_ACT_NONE, st);
    splat_softmax_kernel<<<grid, 256, 0, st>>>(logits, att, N, C, radix, C / groups);
    return launched(ctx);
}

int pcv_splat_combine(pcv_ctx* ctx, const void* x, const float* att, const void* residual, void* y, int N, int HW, int C, int radix,
                      int post_act, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !att || !y || N <= 0 || HW <= 0 || C <= 0 || C % 8 != 0 || radix < 1 || radix > 4 || !dtype_ok(dtype) ||
        post_act < PCV_ACT_NONE || post_act > PCV_ACT_HSWISH)
        return fail(ctx, PCV_ERR_INVALID, "pcv_splat_combine: bad argument (C must be a multiple of 8, radix in [1, 4])");
    const long total8 = (long)N * HW * (C / 8);
    unsigned blocks = 0;
    if (int rc = stream_grid(ctx, "pcv_splat_combine", total8, &blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) {
        splat_combine_kernel<DT_OF(T)><<<blocks, 256, 0, st>>>(x, att, residual, y, total8, HW, C, radix, post_act, ctx->ovf);
    });
    return launched(ctx);
}

// ---- CBAM (cbamresnet.py:48-128): four launches, no tensor of x's size written but y (cbam_kernels.hpp). Like the other aux kernels
// they use static LDS only and are launched directly: nothing to enable, no occupancy slot in the context. -----------------------------
static inline bool cbam_shape_ok(int N, long HW, int C) { return N > 0 && HW > 0 && C >= 8 && C % 8 == 0; }

int pcv_cbam_pool(pcv_ctx* ctx, const void* x, float* s, int N, int HW, int C, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !s || !cbam_shape_ok(N, HW, C) || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_cbam_pool: bad argument (C must be a multiple of 8)");
    hipStream_t st = (hipStream_t)stream;
    dim3 grid((unsigned)N, (unsigned)((C / 8 + 511) / 512));
    for_dtype(dtype, [&](auto T) { cbam_pool_kernel<DT_OF(T)><<<grid, 512, 0, st>>>(x, s, HW, C); });
    return launched(ctx);
}

int pcv_cbam_excite(pcv_ctx* ctx, const float* s, const float* w1, const float* b1, const float* w2, const float* b2, float* mid,
                    float* gate, int N, int C, int M, void* stream) {
    PCV_ENTER(ctx);
    if (!s || !w1 || !b1 || !w2 || !b2 || !mid || !gate || !cbam_shape_ok(N, 1, C) || M < 1 || N > (1 << 30))
        return fail(ctx, PCV_ERR_INVALID, "pcv_cbam_excite: bad argument (C must be a multiple of 8, M >= 1)");
    if ((N + 7) / 8 > 65535) return too_large(ctx, "pcv_cbam_excite", "the batch");
    hipStream_t st = (hipStream_t)stream;
    launch_se_fc(s, w1, b1, mid, 2 * N, C, M, PCV_ACT_RELU, st);          // the mean row and the max row of every image: s is [2N][C]
    dim3 grid((unsigned)((C + 255) / 256), (unsigned)((N + 7) / 8));
    cbam_gate_kernel<<<grid, 256, 0, st>>>(mid, w2, b2, gate, N, C, M);
    return launched(ctx);
}

int pcv_cbam_spatial_pool(pcv_ctx* ctx, const void* x, const float* gate, float* p, int N, int HW, int C, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !gate || !p || !cbam_shape_ok(N, HW, C) || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_cbam_spatial_pool: bad argument (C must be a multiple of 8)");
    int LP = 1;
    while (LP < 64 && LP < C / 8) LP *= 2;                              // lanes of a pixel: min(64, C / 8), as a power of two
    const int slots = 256 / LP;
    // about 16 K elements per block (the gate staging is paid once per block), a whole number of rounds of the block's pixel slots
    int ppb = std::max(slots, 16384 / C);
    ppb = (ppb + slots - 1) / slots * slots;
    const int bpi = (HW + ppb - 1) / ppb;
    unsigned blocks = 0;
    if (int rc = flat_grid(ctx, "pcv_cbam_spatial_pool", (long long)N * bpi, &blocks, 1)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { cbam_spatial_pool_kernel<DT_OF(T)><<<blocks, 256, 0, st>>>(x, gate, p, HW, C, LP, ppb, bpi); });
    return launched(ctx);
}

int pcv_cbam_apply(pcv_ctx* ctx, const void* x, const float* gate, const float* p, const float* w7, const float* scale, const float* shift,
                   const void* residual, void* y, int N, int H, int W, int C, int post_act, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !gate || !p || !w7 || !scale || !shift || !y || N <= 0 || H <= 0 || W <= 0 || C < 8 || C % 8 != 0 || !dtype_ok(dtype) ||
        post_act < PCV_ACT_NONE || post_act > PCV_ACT_HSWISH)
        return fail(ctx, PCV_ERR_INVALID, "pcv_cbam_apply: bad argument (C must be a multiple of 8)");
    if ((long long)H * W > 0x7fffffffll) return too_large(ctx, "pcv_cbam_apply", "the map");
    // A tile: R rows x CW columns, CW == W or R == 1 (a run of consecutive pixels) of about 8 K elements - the four chunks per thread
    // the kernel holds in registers while it computes the tile's gate values - at most kCbamTilePix pixels, so that its 3-pixel
    // halo fits kCbamHalo (cbam_kernels.hpp). The 56 x 56 x 256 map: 32 + 24 pixels of a row, a 7 x 38 halo.
    const int PT = std::min(kCbamTilePix, std::max(4, kCbamPrefetch * 2048 / C));
    CbamApplyParams q;
    if (W <= PT) {
        q.CW = W;
        q.R = std::min(H, PT / W);
    } else {
        q.R = 1;
        q.CW = PT;
    }
    if ((q.R + 6) * (q.CW + 6) > kCbamHalo || q.R * q.CW > kCbamTilePix) return fail(ctx, PCV_ERR_INVALID, "pcv_cbam_apply: tile plan");
    q.tiles_h = (H + q.R - 1) / q.R;
    q.tiles_w = (W + q.CW - 1) / q.CW;
    q.tiles = (long)N * q.tiles_h * q.tiles_w;
    if (q.tiles > 0x7fffffffl) return too_large(ctx, "pcv_cbam_apply", "the grid");
    q.x = x; q.gate = gate; q.p = p; q.w7 = w7; q.res = residual; q.y = y;
    q.scale = scale; q.shift = shift;
    q.H = H; q.W = W; q.C = C;
    q.post_act = post_act;
    q.ovf = ctx->ovf;
    const unsigned blocks = (unsigned)cap_blocks(ctx, q.tiles);
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { cbam_apply_kernel<DT_OF(T)><<<blocks, 256, 0, st>>>(q); });
    return launched(ctx);
}

int pcv_avgpool2d_pad(pcv_ctx* ctx, const void* x, void* y, int N, int H, int W, int C, int k, int s, int p, int ceil_mode,
                      int count_include_pad, int dtype, int out_dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || k <= 0 || s <= 0 || p < 0 || 2 * p > k ||
        !dtype_ok(dtype) || (out_dtype != dtype && out_dtype != PCV_F32))
        return fail(ctx, PCV_ERR_INVALID, "pcv_avgpool2d_pad: bad argument (C must be a multiple of 8, pad <= k/2)");
    if (H + 2 * p < k || W + 2 * p < k) return fail(ctx, PCV_ERR_INVALID, "pcv_avgpool2d_pad: window wider than the padded map");
    const int Ho = pool_out(H, k, s, p, ceil_mode), Wo = pool_out(W, k, s, p, ceil_mode);
    if (Ho <= 0 || Wo <= 0) return fail(ctx, PCV_ERR_INVALID, "pcv_avgpool2d_pad: empty output");
    hipStream_t st = (hipStream_t)stream;
    const int cp = count_include_pad ? 1 : 0;
    return launch_avg(ctx, "pcv_avgpool2d_pad", x, y, N, H, W, C, Ho, Wo, k, s, dtype, out_dtype, st, p, cp, ctx->ovf);
}

int pcv_conv1x1_pair_supported(const pcv_conv_desc* d1, const pcv_conv_desc* d2) {
    return (d1 && d2 && pair_unsupported(*d1, *d2) == nullptr) ? 1 : 0;
}

static int pair_impl(pcv_ctx* ctx, const pcv_conv_desc* d1, const pcv_conv_desc* d2, const void* x, const void* packed1,
                     const float* scale1, const float* shift1, const float* gate, const void* residual, void* y1,
                     const void* packed2, const float* scale2, const float* shift2, void* y2, void* stream);

int pcv_conv1x1_pair_fused(pcv_ctx* ctx, const pcv_conv_desc* d1, const pcv_conv_desc* d2, const void* x, const void* packed1,
                           const float* scale1, const float* shift1, const void* residual, void* y1, const void* packed2,
                           const float* scale2, const float* shift2, void* y2, void* stream) {
    return pair_impl(ctx, d1, d2, x, packed1, scale1, shift1, nullptr, residual, y1, packed2, scale2, shift2, y2, stream);
}

int pcv_conv1x1_pair_gated_supported(const pcv_conv_desc* d1, const pcv_conv_desc* d2) {
    if (!d1 || !d2 || pair_unsupported(*d1, *d2) != nullptr) return 0;
    // kernels that stage the gate rows in LDS hold two images' rows per tile: the map must be at least one tile large
    const int cfg = wpair_cfg(d1->Cin, d1->Cout);
    if (cfg >= 0 && wpair_launch(cfg, d1->dtype, true).gate_in_lds && d1->H * d1->W < wpair_launch(cfg, d1->dtype, true).tileP) return 0;
    return 1;
}

int pcv_conv1x1_pair_gated_fused(pcv_ctx* ctx, const pcv_conv_desc* d1, const pcv_conv_desc* d2, const void* x,
                                 const void* packed1, const float* scale1, const float* shift1, const float* gate,
                                 const void* residual, void* y1, const void* packed2, const float* scale2, const float* shift2,
                                 void* y2, void* stream) {
    if (!ctx) return PCV_ERR_INVALID;
    if (!gate || !aligned16(gate) || !pcv_conv1x1_pair_gated_supported(d1, d2))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_gated_fused: unsupported pair or missing gate");
    return pair_impl(ctx, d1, d2, x, packed1, scale1, shift1, gate, residual, y1, packed2, scale2, shift2, y2, stream);
}

static int pair_impl(pcv_ctx* ctx, const pcv_conv_desc* d1, const pcv_conv_desc* d2, const void* x, const void* packed1,
                     const float* scale1, const float* shift1, const float* gate, const void* residual, void* y1,
                     const void* packed2, const float* scale2, const float* shift2, void* y2, void* stream) {
    PCV_ENTER(ctx);
    if (!d1 || !d2 || !x || !packed1 || !scale1 || !shift1 || !residual || !y1 || !packed2 || !scale2 || !shift2 || !y2)
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_fused: NULL argument");
    if (const char* why = pair_unsupported(*d1, *d2)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_conv1x1_pair_fused: ") + why);
    if (!aligned16(x) || !aligned16(packed1) || !aligned16(packed2) || !aligned16(residual) || !aligned16(y1) || !aligned16(y2))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_fused: pointers must be 16-byte aligned");
    ConvPlan P1, P2;
    const char* why = plan_conv(*d1, P1, false);
    if (!why) why = plan_conv(*d2, P2, false);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_conv1x1_pair_fused: ") + why);
    const long M = (long)d1->N * d1->H * d1->W;
    hipStream_t st = (hipStream_t)stream;
    if (d1->Cin >= 128) {
        const int CM = d1->Cin, C1 = d1->Cout, cfg = wpair_cfg(CM, C1);
        if (cfg < 0 || P1.wrows != C1 || P1.Kpad != CM || P2.wrows != CM || P2.Kpad != C1 || P1.ngb != 1 || P2.ngb != 1)
            return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_fused: unexpected packed layout");
        WPairParams q;
        std::memset(&q, 0, sizeof(q));
        q.x = x; q.res = residual; q.y1 = y1; q.y2 = y2; q.ovf = ctx->ovf;
        q.w1 = static_cast<const char*>(packed1) + P1.ktab_bytes;
        q.w2 = static_cast<const char*>(packed2) + P2.ktab_bytes;
        q.scale1 = scale1; q.shift1 = shift1; q.scale2 = scale2; q.shift2 = shift2;
        q.x_bytes = q.y2_bytes = (uint32_t)(M * CM * 2); q.res_bytes = q.y1_bytes = (uint32_t)(M * C1 * 2);
        q.w1_bytes = q.w2_bytes = (uint32_t)(C1 * CM * 2);
        const WPairLaunch L = wpair_launch(cfg, d1->dtype, gate != nullptr);
        q.gate = gate;
        q.div_hw = make_fastdiv((uint32_t)(d1->H * d1->W));
        q.hw = (uint32_t)(d1->H * d1->W);
        q.M = (int)M; q.nTiles = (int)((M + L.tileP - 1) / L.tileP);
        q.act1 = d1->act; q.post1 = d1->post_act; q.act2 = d2->act;
        const unsigned grid = (unsigned)std::min<long>(q.nTiles, (long)block_slots(ctx, ctx->wpair_bpc[cfg]));
        return launch(ctx, L.k, grid, st, q);
    }
    if (P1.wrows != 256 || P1.Kpad != 64 || P2.wrows != 64 || P2.Kpad != 256 || P1.ngb != 1 || P2.ngb != 1)
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_fused: unexpected packed layout");
    PairParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.res = residual; p.y1 = y1; p.y2 = y2; p.ovf = ctx->ovf;
    p.w1 = static_cast<const char*>(packed1) + P1.ktab_bytes;
    p.w2 = static_cast<const char*>(packed2) + P2.ktab_bytes;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = scale2; p.shift2 = shift2;
    p.x_bytes = (uint32_t)(M * 64 * 2); p.res_bytes = p.y1_bytes = (uint32_t)(M * 256 * 2); p.y2_bytes = (uint32_t)(M * 64 * 2);
    p.w1_bytes = 256 * 64 * 2; p.w2_bytes = 64 * 256 * 2;
    const int pb = ctx->pair_pb == 4 ? 4 : 2;
    p.M = (int)M; p.nTiles = (int)((M + 16 * pb - 1) / (16 * pb));
    p.act1 = d1->act; p.post1 = d1->post_act; p.act2 = d2->act;
    p.gate = gate;
    p.div_hw = make_fastdiv((uint32_t)(d1->H * d1->W));
    const PairForm form = gate ? PAIR_GATED : (pb == 4 ? PAIR_PB4 : PAIR_PB2);
    if (gate) p.nTiles = (int)((M + 31) / 32);          // the gated form is instantiated for PB == 2 only
    const unsigned grid = (unsigned)std::min<long>(p.nTiles, (long)block_slots(ctx, ctx->pair_bpc[form == PAIR_PB4 ? 0 : 1]));
    return launch(ctx, kPair[d1->dtype == PCV_BF16 ? 0 : 1][form], grid, st, p);
}

static const char* pair_idconv_unsupported(const pcv_conv_desc& di, const pcv_conv_desc& a, const pcv_conv_desc& b) {
    if (desc_stale(di)) return kStaleDesc;
    if (const char* why = pair_unsupported(a, b)) return why;
    if (a.Cin != 64) return "identity-convolution variant: only the 64 -> 256 -> 64 pair is instantiated";
    if (!plain_1x1(di) || di.dtype != a.dtype) return "identity convolution must be a plain 1x1 stride 1 of the same dtype";
    if (di.N != a.N || di.H != a.H || di.W != a.W || di.Cin != 64 || di.Cout != a.Cout) return "identity convolution shapes do not match";
    if (di.act != PCV_ACT_NONE || di.has_residual || di.post_act != PCV_ACT_NONE) return "identity convolution must have no activation";
    return nullptr;
}

int pcv_conv1x1_pair_idconv_supported(const pcv_conv_desc* d_id, const pcv_conv_desc* d1, const pcv_conv_desc* d2) {
    return (d_id && d1 && d2 && pair_idconv_unsupported(*d_id, *d1, *d2) == nullptr) ? 1 : 0;
}

int pcv_conv1x1_pair_idconv_fused(pcv_ctx* ctx, const pcv_conv_desc* d_id, const pcv_conv_desc* d1, const pcv_conv_desc* d2,
                                  const void* x0, const void* packed_id, const float* scale_id, const float* shift_id,
                                  const void* x, const void* packed1, const float* scale1, const float* shift1, void* y1,
                                  const void* packed2, const float* scale2, const float* shift2, void* y2, void* stream) {
    PCV_ENTER(ctx);
    if (!d_id || !d1 || !d2 || !x0 || !packed_id || !scale_id || !shift_id || !x || !packed1 || !scale1 || !shift1 || !y1 ||
        !packed2 || !scale2 || !shift2 || !y2)
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_idconv_fused: NULL argument");
    if (const char* why = pair_idconv_unsupported(*d_id, *d1, *d2))
        return fail(ctx, PCV_ERR_INVALID, std::string("pcv_conv1x1_pair_idconv_fused: ") + why);
    if (!aligned16(x0) || !aligned16(packed_id) || !aligned16(x) || !aligned16(packed1) || !aligned16(packed2) || !aligned16(y1) ||
        !aligned16(y2))
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_idconv_fused: pointers must be 16-byte aligned");
    ConvPlan Pi, P1, P2;
    const char* why = plan_conv(*d_id, Pi, false);
    if (!why) why = plan_conv(*d1, P1, false);
    if (!why) why = plan_conv(*d2, P2, false);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_conv1x1_pair_idconv_fused: ") + why);
    if (P1.wrows != 256 || P1.Kpad != 64 || P2.wrows != 64 || P2.Kpad != 256 || Pi.wrows != 256 || Pi.Kpad != 64 || P1.ngb != 1 ||
        P2.ngb != 1 || Pi.ngb != 1)
        return fail(ctx, PCV_ERR_INVALID, "pcv_conv1x1_pair_idconv_fused: unexpected packed layout");
    PairParams p;
    std::memset(&p, 0, sizeof(p));
    const long M = (long)d1->N * d1->H * d1->W;
    p.x = x; p.res = nullptr; p.y1 = y1; p.y2 = y2; p.x0 = x0; p.ovf = ctx->ovf;
    p.w1 = static_cast<const char*>(packed1) + P1.ktab_bytes;
    p.w2 = static_cast<const char*>(packed2) + P2.ktab_bytes;
    p.wid = static_cast<const char*>(packed_id) + Pi.ktab_bytes;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = scale2; p.shift2 = shift2; p.scale_id = scale_id; p.shift_id = shift_id;
    p.x_bytes = p.x0_bytes = (uint32_t)(M * 64 * 2); p.res_bytes = 0; p.y1_bytes = (uint32_t)(M * 256 * 2); p.y2_bytes = (uint32_t)(M * 64 * 2);
    p.w1_bytes = p.wid_bytes = 256 * 64 * 2; p.w2_bytes = 64 * 256 * 2;
    p.M = (int)M; p.nTiles = (int)((M + 31) / 32);
    p.act1 = d1->act; p.post1 = d1->post_act; p.act2 = d2->act;
    const unsigned grid = (unsigned)std::min<long>(p.nTiles, (long)block_slots(ctx, ctx->pair_idc_bpc));
    return launch(ctx, kPair[d1->dtype == PCV_BF16 ? 0 : 1][PAIR_IDCONV], grid, (hipStream_t)stream, p);
}

// Which bottleneck units the fused kernel (bnu.hpp) covers: 16 bit, 56-wide maps, 1x1 (256 | 64 with an identity convolution) -> 64,
// 3x3 / s1 / p1 64 -> 64, 1x1 64 -> 256 with the skip add; clamp activations only. Shape and dtype decide, never the batch size.
static const char* bottleneck_unsupported(const pcv_conv_desc& a, const pcv_conv_desc& b, const pcv_conv_desc& c, const pcv_conv_desc* di) {
    if (desc_stale(a) || desc_stale(b) || desc_stale(c) || (di && desc_stale(*di))) return kStaleDesc;
    if (g_bnu == 0) return "switched off (pcv_set_tuning(\"bnu\", 0))";
    if (a.dtype != PCV_BF16 && a.dtype != PCV_F16) return "16-bit storage only";
    if (b.dtype != a.dtype || c.dtype != a.dtype || (di && di->dtype != a.dtype)) return "one storage type for the whole unit";
    if (!plain_1x1(a) || !plain_1x1(c) || (di && !plain_1x1(*di))) return "conv1, conv3 and the identity convolution must be plain 1x1 stride 1";
    const bool b3x3 = b.kh == 3 && b.kw == 3 && b.stride_h == 1 && b.stride_w == 1 && b.dil_h == 1 && b.dil_w == 1 && b.pad_t == 1 &&
                      b.pad_l == 1 && b.pad_b == 1 && b.pad_r == 1 && b.groups == 1 && b.out_dtype == b.dtype &&
                      (b.x_cpitch == 0 || b.x_cpitch == b.Cin) && (b.x_wpitch == 0 || b.x_wpitch == b.W) && (b.y_cpitch == 0 || b.y_cpitch == b.Cout);
    if (!b3x3) return "conv2 must be a dense 3x3, stride 1, pad 1";
    if (a.Cin != (di ? 64 : 256) || a.Cout != 64 || b.Cin != 64 || b.Cout != 64 || c.Cin != 64 || c.Cout != 256)
        return "only 256 -> 64 -> 64 -> 256 (64 -> .. with an identity convolution) is instantiated";
    if (a.W != BnuCfg<false>::W || a.N < 1 || a.H < 1) return "56-wide maps only";
    if (b.N != a.N || b.H != a.H || b.W != a.W || c.N != a.N || c.H != a.H || c.W != a.W) return "shapes do not chain";
    if (a.has_residual || a.post_act != PCV_ACT_NONE || b.has_residual || b.post_act != PCV_ACT_NONE || !c.has_residual)
        return "conv3 carries the skip add, conv1 and conv2 do not";
    if (a.act > PCV_ACT_RELU6 || b.act > PCV_ACT_RELU6 || c.act > PCV_ACT_RELU6 || c.post_act > PCV_ACT_RELU6 || a.act < 0 || b.act < 0 ||
        c.act < 0 || c.post_act < 0)
        return "clamp activations only (none / ReLU / ReLU6)";
    if (di) {
        if (di->N != a.N || di->H != a.H || di->W != a.W || di->Cin != 64 || di->Cout != 256) return "identity convolution shapes do not match";
        if (di->act != PCV_ACT_NONE || di->has_residual || di->post_act != PCV_ACT_NONE) return "identity convolution must have no activation";
    }
    if ((long)a.N * a.H * a.W * c.Cout * 2 >= (1L << 31)) return kTensorTooLarge;
    return nullptr;
}

int pcv_bottleneck_supported(const pcv_conv_desc* d1, const pcv_conv_desc* d2, const pcv_conv_desc* d3, const pcv_conv_desc* d_id) {
    return (d1 && d2 && d3 && bottleneck_unsupported(*d1, *d2, *d3, d_id) == nullptr) ? 1 : 0;
}

int pcv_bottleneck_fused(pcv_ctx* ctx, const pcv_conv_desc* d1, const pcv_conv_desc* d2, const pcv_conv_desc* d3, const pcv_conv_desc* d_id,
                         const void* x, const void* packed1, const float* scale1, const float* shift1, const void* packed2,
                         const float* scale2, const float* shift2, const void* packed3, const float* scale3, const float* shift3,
                         const void* packed_id, const float* scale_id, const float* shift_id, void* y, void* stream) {
    PCV_ENTER(ctx);
    if (!d1 || !d2 || !d3 || !x || !packed1 || !scale1 || !shift1 || !packed2 || !scale2 || !shift2 || !packed3 || !scale3 || !shift3 || !y ||
        (d_id && (!packed_id || !scale_id || !shift_id)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_bottleneck_fused: NULL argument");
    if (const char* why = bottleneck_unsupported(*d1, *d2, *d3, d_id)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_bottleneck_fused: ") + why);
    if (!aligned16(x) || !aligned16(packed1) || !aligned16(packed2) || !aligned16(packed3) || !aligned16(y) || (d_id && !aligned16(packed_id)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_bottleneck_fused: pointers must be 16-byte aligned");
    ConvPlan P1, P2, P3, Pi;
    const char* why = plan_conv(*d1, P1, false);
    if (!why) why = plan_conv(*d2, P2, false);
    if (!why) why = plan_conv(*d3, P3, false);
    if (!why && d_id) why = plan_conv(*d_id, Pi, false);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_bottleneck_fused: ") + why);
    if (P1.wrows != 64 || P1.Kpad != d1->Cin || !P2.conv3 || P2.wrows != 64 || P2.Kpad != 9 * 64 || P3.wrows != 256 || P3.Kpad != 64 ||
        P1.ngb != 1 || P2.ngb != 1 || P3.ngb != 1 || (d_id && (Pi.wrows != 256 || Pi.Kpad != 64 || Pi.ngb != 1)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_bottleneck_fused: unexpected packed layout");
    BnuParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.ovf = ctx->ovf;
    p.w1 = static_cast<const char*>(packed1) + P1.ktab_bytes;
    p.w2 = static_cast<const char*>(packed2) + P2.ktab_bytes;
    p.w3 = static_cast<const char*>(packed3) + P3.ktab_bytes;
    p.scale1 = scale1; p.shift1 = shift1; p.scale2 = scale2; p.shift2 = shift2; p.scale3 = scale3; p.shift3 = shift3;
    p.w1_bytes = (uint32_t)(64 * d1->Cin * 2); p.w2_bytes = 64 * 9 * 64 * 2; p.w3_bytes = 256 * 64 * 2;
    if (d_id) {
        p.wid = static_cast<const char*>(packed_id) + Pi.ktab_bytes;
        p.wid_bytes = 256 * 64 * 2;
        p.scale_id = scale_id; p.shift_id = shift_id;
    }
    p.N = d1->N; p.H = d1->H;
    p.y_bytes = (uint32_t)((long)d1->N * d1->H * d1->W * 256 * 2);
    // Items = (image, band of rows): whole images once they fill the chip, else bands of at least 4 rows (each band recomputes conv1 on
    // its two halo rows). The split changes which block computes a row, never the row's value.
    int band = d1->H;
    if (ctx->bnu_band > 0) band = std::min(ctx->bnu_band, d1->H);
    else if (d1->N < ctx->num_cu) {
        const int nb = std::max(1, std::min((d1->H + 3) / 4, (ctx->num_cu + d1->N - 1) / d1->N));
        band = (d1->H + nb - 1) / nb;
    }
    p.band = band; p.nBands = (d1->H + band - 1) / band;
    const long long items = (long long)d1->N * p.nBands;
    if (items >= 0x7FFFFFFFll) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_bottleneck_fused: too many items; split the batch");
    p.nItems = (int)items;
    p.act1 = d1->act; p.act2 = d2->act; p.act3 = d3->act; p.post3 = d3->post_act;
    const unsigned grid = (unsigned)std::min<long long>(items, block_slots(ctx, 1));
    return launch(ctx, kBnu[d1->dtype == PCV_BF16 ? 0 : 1][d_id ? 1 : 0], grid, (hipStream_t)stream, p);
}

int pcv_channel_slice(pcv_ctx* ctx, const void* x, void* y, long rows, int C, int offset, int x_cpitch, int y_cpitch, int dtype,
                      void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || rows <= 0 || C <= 0 || offset < 0 || x_cpitch < offset + C || y_cpitch < C || y_cpitch % 8 != 0 || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_channel_slice: bad argument (y_cpitch must be a multiple of 8 and hold C channels)");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_channel_slice", (long long)rows * (y_cpitch / 8), &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { channel_slice_kernel<DT_OF(T)><<<grid, 256, 0, st>>>(x, y, rows, C, offset, x_cpitch, y_cpitch); });
    return launched(ctx);
}

int pcv_channel_concat(pcv_ctx* ctx, const void* x, void* y, long rows, int C, int x_cpitch, int y_cpitch, int y_offset, int dtype,
                       void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || rows <= 0 || C <= 0 || C % 8 != 0 || x_cpitch < C || x_cpitch % 8 != 0 || y_offset < 0 || y_offset % 8 != 0 ||
        y_cpitch < y_offset + C || y_cpitch % 8 != 0 || !dtype_ok(dtype) || !aligned16(x) || !aligned16(y))
        return fail(ctx, PCV_ERR_INVALID, "pcv_channel_concat: bad argument (C, offset and pitches must be multiples of 8, y must hold the slice)");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_channel_concat", (long long)rows * (C / 8), &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { channel_concat_kernel<DT_OF(T)><<<grid, 256, 0, st>>>(x, y, rows, C, x_cpitch, y_cpitch, y_offset); });
    return launched(ctx);
}

int pcv_interpolate(pcv_ctx* ctx, const void* x, void* y, int N, int H, int W, int C, int Ho, int Wo, int bilinear,
                    int align_corners, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8 != 0 || Ho <= 0 || Wo <= 0 || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_interpolate: bad argument (C must be a multiple of 8)");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_interpolate", (long long)N * Ho * Wo * (C / 8), &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { interpolate_kernel<DT_OF(T)><<<grid, 256, 0, st>>>(x, y, N, H, W, C, Ho, Wo, bilinear, align_corners); });
    return launched(ctx);
}

// ---- HRNet's multi-resolution fuse (hrnet.py:40-47,126-134; hrfuse.hpp) --------------------------------------------------------------
// every check that needs no pointer and no context: PCV_OK, or the code with the reason in *why
static int check_hr_fuse(int nsrc, const int* shift, int N, int H, int W, int C, int act, int dtype, const char** why) {
    *why = nullptr;
    if (nsrc < 1 || nsrc > kHrMaxSrc) *why = "needs 1 .. 4 sources";
    else if (!shift) *why = "NULL shift array";
    else if (!dtype_ok(dtype)) *why = "unknown dtype";
    else if (act != PCV_ACT_NONE && act != PCV_ACT_RELU) *why = "the activation must be PCV_ACT_NONE or PCV_ACT_RELU";
    else if (N <= 0 || H <= 0 || W <= 0 || C <= 0) *why = "empty output";
    else if (C % 8 != 0) *why = "C (the physical channel pitch) must be a multiple of 8";
    if (*why) return PCV_ERR_INVALID;
    for (int t = 0; t < nsrc; ++t) {
        if (shift[t] < 0 || shift[t] > kHrMaxShift) { *why = "a shift must be in 0 .. 3"; return PCV_ERR_INVALID; }
        const int m = (1 << shift[t]) - 1;
        if ((H & m) != 0 || (W & m) != 0) { *why = "H and W must be exact multiples of 1 << shift (the size does not divide)"; return PCV_ERR_INVALID; }
    }
    // (factor by factor: the product of four ints does not fit 64 bits)
    unsigned long long ybytes = (unsigned long long)N * (unsigned long long)H;
    if (in_window(ybytes)) ybytes *= (unsigned long long)W;
    if (in_window(ybytes)) ybytes *= (unsigned long long)C * esize(dtype);
    if (!in_window(ybytes)) { *why = kTensorTooLarge; return PCV_ERR_TOO_LARGE; }
    return PCV_OK;
}

int pcv_hr_fuse_supported(int nsrc, const int* shift, int N, int H, int W, int C, int act, int dtype) {
    const char* why = nullptr;
    if (check_hr_fuse(nsrc, shift, N, H, W, C, act, dtype, &why) != PCV_OK) {
        fail(nullptr, PCV_ERR_INVALID, std::string("pcv_hr_fuse_supported: ") + why);
        return 0;
    }
    return 1;
}

int pcv_hr_fuse(pcv_ctx* ctx, const void* const* src, const int* shift, int nsrc, void* y, int N, int H, int W, int C, int act,
                int dtype, void* stream) {
    PCV_ENTER(ctx);
    const char* why = nullptr;
    if (int rc = check_hr_fuse(nsrc, shift, N, H, W, C, act, dtype, &why)) return fail(ctx, rc, std::string("pcv_hr_fuse: ") + why);
    if (!src || !y) return fail(ctx, PCV_ERR_INVALID, "pcv_hr_fuse: NULL argument");
    HrFuseParams p = {};
    for (int t = 0; t < nsrc; ++t) {
        if (!src[t]) return fail(ctx, PCV_ERR_INVALID, "pcv_hr_fuse: NULL source pointer");
        if (src[t] == y) return fail(ctx, PCV_ERR_INVALID, "pcv_hr_fuse: y must not be one of the sources (not an in-place operation)");
        if (!aligned16(src[t])) return fail(ctx, PCV_ERR_INVALID, "pcv_hr_fuse: pointers must be 16-byte aligned");
        p.src[t] = src[t];
        p.shift[t] = shift[t];
    }
    if (!aligned16(y)) return fail(ctx, PCV_ERR_INVALID, "pcv_hr_fuse: pointers must be 16-byte aligned");
    p.y = y;
    p.H = H; p.W = W; p.C8 = C / 8;
    p.dC8 = make_fastdiv((uint32_t)p.C8);
    p.dW = make_fastdiv((uint32_t)W);
    p.dH = make_fastdiv((uint32_t)H);
    const long long total = (long long)N * H * W * p.C8;             // one thread per 8-channel chunk; < 2^27: y fits the 2 GiB window
    p.total = (uint32_t)total;
    p.act = act;
    p.ovf = ctx->ovf;
    unsigned grid = 0;
    if (int rc = stream_grid(ctx, "pcv_hr_fuse", total, &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { launch_hr_fuse<DT_OF(T)>(nsrc, grid, st, p); });
    return launched(ctx);
}

int pcv_channel_interleave2(pcv_ctx* ctx, const void* a, const void* b, void* y, long rows, int Ch, int a_cpitch, int b_cpitch,
                            int y_cpitch, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!a || !b || !y || rows <= 0 || Ch <= 0 || a_cpitch < Ch || b_cpitch < Ch || y_cpitch < 2 * Ch || y_cpitch % 8 != 0 ||
        !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_channel_interleave2: bad argument (y_cpitch must be a multiple of 8 and hold 2*Ch channels)");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_channel_interleave2", (long long)rows * (y_cpitch / 8), &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) {
        channel_interleave2_kernel<DT_OF(T)><<<grid, 256, 0, st>>>(a, b, y, rows, Ch, a_cpitch, b_cpitch, y_cpitch);
    });
    return launched(ctx);
}

int pcv_preprocess_u8(pcv_ctx* ctx, const unsigned char* x, void* y, int N, int Hs, int Ws, int C, int top, int left, int H,
                      int W, int wpitch, const float* mean, const float* inv_std, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!x || !y || !mean || !inv_std || N <= 0 || Hs <= 0 || Ws <= 0 || C <= 0 || C > 4 || H <= 0 || W <= 0 || top < 0 ||
        left < 0 || top + H > Hs || left + W > Ws || wpitch < W || !dtype_ok(dtype))
        return fail(ctx, PCV_ERR_INVALID, "pcv_preprocess_u8: bad argument (C <= 4, crop inside the frame, wpitch >= W)");
    unsigned grid = 0;
    if (int rc = flat_grid(ctx, "pcv_preprocess_u8", (long long)N * H * wpitch, &grid)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) {
        preprocess_u8_kernel<DT_OF(T)><<<grid, 256, 0, st>>>(x, y, N, Hs, Ws, C, top, left, H, W, 4, wpitch, mean, inv_std, ctx->ovf);
    });
    return launched(ctx);
}

// Resize + crop + normalise of ragged frames (resize_plan.hpp, resize_kernel.hpp). The two planning calls are host arithmetic only:
// no context, no device; their refusals leave the text where pcv_last_error(NULL) finds it.
int pcv_resize_plan_bytes(int N, const int* hs, const int* ws, int C, int size, int H, int W, size_t* bytes) {
    if (!bytes) return fail(nullptr, PCV_ERR_INVALID, "pcv_resize_plan_bytes: bytes is NULL");
    *bytes = 0;
    if (const char* why = pcv_resize::plan_bytes(N, hs, ws, C, size, H, W, bytes))
        return fail(nullptr, PCV_ERR_INVALID, std::string("pcv_resize_plan_bytes: ") + why);
    return PCV_OK;
}

int pcv_resize_plan(const void* const* frames, int N, const int* hs, const int* ws, int C, int size, int H, int W, void* blob,
                    size_t bytes) {
    if (const char* why = pcv_resize::plan(frames, N, hs, ws, C, size, H, W, blob, bytes))
        return fail(nullptr, PCV_ERR_INVALID, std::string("pcv_resize_plan: ") + why);
    return PCV_OK;
}

int pcv_resize_crop_u8(pcv_ctx* ctx, const void* plan_host, const void* plan_dev, size_t bytes, void* y, int wpitch,
                       const float* mean, const float* inv_std, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (!plan_host || !plan_dev || !y || !mean || !inv_std || !dtype_ok(dtype) || !aligned16(plan_dev) || !aligned16(y))
        return fail(ctx, PCV_ERR_INVALID, "pcv_resize_crop_u8: bad argument (NULL pointer, dtype, or plan_dev / y not 16-byte aligned)");
    if (const char* why = pcv_resize::validate(plan_host, bytes)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_resize_crop_u8: ") + why);
    pcv_resize::ResizeHeader hd;
    std::memcpy(&hd, plan_host, sizeof(hd));
    if (wpitch < hd.W) return fail(ctx, PCV_ERR_INVALID, "pcv_resize_crop_u8: wpitch < W");
    if (!in_window((unsigned long long)hd.N * hd.H * wpitch * 4 * esize(dtype))) return too_large(ctx, "pcv_resize_crop_u8", "y");
    const unsigned blocks = (unsigned)cap_blocks(ctx, hd.items);            // a fresh block per (frame, band): see resize_kernel.hpp
    const char* pd = static_cast<const char*>(plan_dev);
    hipStream_t st = (hipStream_t)stream;
    const unsigned lds = (unsigned)hd.stage_bytes;
    for_dtype(dtype, [&](auto T) { resize_crop_u8_kernel<DT_OF(T)><<<blocks, 256, lds, st>>>(pd, y, wpitch, mean, inv_std, ctx->ovf); });
    return launched(ctx);
}

int pcv_classify_f32(pcv_ctx* ctx, const float* logits, int N, int J, int k, int* top_idx, float* top_val, float* top_prob,
                     const long long* labels, int* rank, float* nll, void* stream) {
    PCV_ENTER(ctx);
    if (!logits) return fail(ctx, PCV_ERR_INVALID, "pcv_classify_f32: logits is NULL");
    if (N < 1) return fail(ctx, PCV_ERR_INVALID, "pcv_classify_f32: N = " + std::to_string(N) + " is outside the limit N >= 1");
    if (J < 1 || J > kClassifyMaxJ)
        return fail(ctx, PCV_ERR_INVALID, "pcv_classify_f32: J = " + std::to_string(J) + " is outside the limit 1 <= J <= 16384 (a row is staged in 64 KB of LDS)");
    if (k < 0 || k > std::min(J, kClassifyMaxK))
        return fail(ctx, PCV_ERR_INVALID, "pcv_classify_f32: k = " + std::to_string(k) + " is outside the limit 0 <= k <= min(J, 32) (J = " + std::to_string(J) + ")");
    if (k == 0 && (top_idx || top_val || top_prob))
        return fail(ctx, PCV_ERR_INVALID, "pcv_classify_f32: k = 0 is allowed only when top_idx, top_val and top_prob are all NULL");
    if ((rank || nll) && !labels) return fail(ctx, PCV_ERR_INVALID, "pcv_classify_f32: rank and nll need labels");
    const long long blocks = cap_blocks(ctx, N);
    const Kernel K = classify_kernel_of(J);
    void* args[] = {&logits, &N, &J, &k, &top_idx, &top_val, &top_prob, &labels, &rank, &nll};
    HIP_TRY(ctx, hipLaunchKernel(K.fn, dim3((unsigned)blocks), dim3((unsigned)K.threads), args, (size_t)K.lds, (hipStream_t)stream));
    return PCV_OK;
}

int pcv_mbconv_supported(const pcv_conv_desc* d_exp, const pcv_conv_desc* d_dw, const pcv_conv_desc* d_proj) {
    return (d_dw && d_proj && mbconv_unsupported(d_exp, *d_dw, *d_proj) == nullptr) ? 1 : 0;
}

int pcv_mbconv_fused(pcv_ctx* ctx, const pcv_conv_desc* d_exp, const pcv_conv_desc* d_dw, const pcv_conv_desc* d_proj,
                     const void* x, const void* packed_exp, const float* scale_e, const float* shift_e, const void* packed_dw,
                     const float* scale_d, const float* shift_d, const void* packed_proj, const float* scale_p,
                     const float* shift_p, const void* residual, void* y, void* stream) {
    PCV_ENTER(ctx);
    if (!d_dw || !d_proj || !x || !packed_dw || !scale_d || !shift_d || !packed_proj || !scale_p || !shift_p || !y ||
        (d_exp && (!packed_exp || !scale_e || !shift_e)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: NULL argument");
    if (const char* why = mbconv_unsupported(d_exp, *d_dw, *d_proj)) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_mbconv_fused: ") + why);
    if (d_proj->has_residual && !residual) return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: has_residual but residual is NULL");
    if (!aligned16(x) || !aligned16(packed_dw) || !aligned16(packed_proj) || !aligned16(y) || (d_exp && !aligned16(packed_exp)) ||
        (residual && !aligned16(residual)) || !aligned16(scale_d) || !aligned16(shift_d) || !aligned16(scale_p) || !aligned16(shift_p) ||
        (d_exp && (!aligned16(scale_e) || !aligned16(shift_e))))
        return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: pointers must be 16-byte aligned");
    ConvPlan Pe, Pp;
    const char* why = d_exp ? plan_conv(*d_exp, Pe, false) : nullptr;
    if (!why) why = plan_conv(*d_proj, Pp, false);
    if (why) return fail(ctx, PCV_ERR_INVALID, std::string("pcv_mbconv_fused: ") + why);
    if (Pp.ngb != 1 || (d_exp && Pe.ngb != 1)) return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: unexpected packed layout");
    MbParams p;
    std::memset(&p, 0, sizeof(p));
    const int S = d_dw->stride_h;
    p.x = x; p.res = d_proj->has_residual ? residual : nullptr; p.y = y; p.ovf = ctx->ovf;
    p.dbg = reinterpret_cast<uint32_t*>(ctx->dbg_ptr);
    p.w_exp = d_exp ? static_cast<const char*>(packed_exp) + Pe.ktab_bytes : nullptr;
    p.w_dw = packed_dw;
    p.w_dwsp = static_cast<const char*>(packed_dw) + dw_taps_bytes(*d_dw);                // (present for 16-bit 3x3: checked by mbconv_unsupported)
    p.w_proj = static_cast<const char*>(packed_proj) + Pp.ktab_bytes;
    p.scale_e = scale_e; p.shift_e = shift_e; p.scale_d = scale_d; p.shift_d = shift_d; p.scale_p = scale_p; p.shift_p = shift_p;
    p.N = d_dw->N; p.H = d_dw->H; p.W = d_dw->W; p.Cmid = d_dw->Cin; p.Cin = d_exp ? d_exp->Cin : p.Cmid; p.Cout = d_proj->Cout;
    p.Ho = (p.H - 1) / S + 1; p.Wo = (p.W - 1) / S + 1;
    p.x_bytes = (uint32_t)((long)p.N * p.H * p.W * p.Cin * 2);
    p.y_bytes = (uint32_t)((long)p.N * p.Ho * p.Wo * p.Cout * 2);
    p.wexp_bytes = d_exp ? (uint32_t)Pe.w_bytes : 0;
    p.wdw_bytes = (uint32_t)(9 * p.Cmid * 2);
    p.wproj_bytes = (uint32_t)Pp.w_bytes;
    p.Kpad1 = d_exp ? Pe.Kpad : 0; p.Kpad2 = Pp.Kpad;
    p.ka = d_exp ? (p.Cin + 31) / 32 : 0;
    p.nChunks = (p.Cmid + 31) / 32;
    p.nRowT = Pp.wrows / 16;
    const int TH = S == 1 ? 8 : 4;
    p.tilesH = (p.Ho + TH - 1) / TH; p.tilesW = (p.Wo + 15) / 16;
    p.nTiles = p.N * p.tilesH * p.tilesW;
    p.act_e = d_exp ? d_exp->act : 0; p.act_d = d_dw->act; p.act_p = d_proj->act; p.post = d_proj->post_act;
    if ((d_exp && p.Kpad1 < 32 * p.ka) || p.Kpad2 < 32 * p.nChunks)
        return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: unexpected packed layout");
    // wave-private tiles (mbw.hpp) where the unit qualifies; pcv_set_tuning("mbw", 0) sends the shapes BOTH kernels cover to mbconv.hpp
    int kaw = 0, nrt = 0, rbw = 0;
    const bool wave_shape = d_exp && mbw_shape(p.Cin, p.Cout, S, p.H, p.W, &kaw, &nrt, &rbw);
    const bool block_shape = p.Cout <= 32 && p.Wo >= 24;
    // register-resident tiles (mbr.hpp): one expand K step, the unit's weights + diagonal fragments in LDS
    if (wave_shape && ctx->use_mbr) {
        const MbrEntry* e = pick_mbr(ctx, d_dw->dtype, nrt, p.act_e == p.act_d ? p.act_e : -1, S, kaw, p.nChunks);
        if (e) {
            const int oc = mbr_out_cols(S, e->nrt);                             // output columns of a wave tile
            p.tilesH = (p.Ho + e->ro - 1) / e->ro; p.tilesW = (p.Wo + oc - 1) / oc;
            const long nT = (long)p.N * p.tilesH * p.tilesW;
            if (nT >= 0x7FFFFFFFl) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_mbconv_fused: too many tiles; split the batch");
            p.nTiles = (int)nT;
            const unsigned gridr = (unsigned)std::min<long>((nT + e->waves - 1) / e->waves, (long)block_slots(ctx, 1));
            return launch(ctx, mbr_kernel_of(*e, mbr_entry_lds(*e, p.nChunks)), gridr, (hipStream_t)stream, p);
        }
    }
    if (wave_shape && (ctx->use_mbw || !block_shape)) {
        // pixel-block shape: 1 x 16 or 2 x 8 outputs, whichever covers the map with less expand work (window blocks x tiles)
        const int nblk = rbw > 0 ? rbw : (S == 1 ? 4 : 2);
        auto tiles_of = [&](int tw) { return (long)((p.Ho + nblk * (16 / tw) - 1) / (nblk * (16 / tw))) * ((p.Wo + tw - 1) / tw); };
        int tw = mbw_npt(S, 8, rbw) * tiles_of(8) < mbw_npt(S, 16, rbw) * tiles_of(16) ? 8 : 16;
        if (ctx->use_mbw == 8 || ctx->use_mbw == 16) tw = ctx->use_mbw;
        if (rbw > 0) tw = 16;                                   // the wide units are instantiated for 1 x 16 pixel blocks only
        const int nw = mbw_waves(S, nrt, p.nChunks, tw, kaw, rbw);
        if (nw > 0) {
            const int RO = nblk * (16 / tw);
            p.tilesH = (p.Ho + RO - 1) / RO; p.tilesW = (p.Wo + tw - 1) / tw;
            const long nT = (long)p.N * p.tilesH * p.tilesW;
            if (nT >= 0x7FFFFFFFl) return fail(ctx, PCV_ERR_TOO_LARGE, "pcv_mbconv_fused: too many tiles; split the batch");
            p.nTiles = (int)nT;
            const MbwLds wl = mbw_lds_layout(S, nrt, p.nChunks, nw, tw, kaw, rbw);
            const long want = (nT + nw - 1) / nw;
            const unsigned gridw = (unsigned)std::min<long>(want, (long)block_slots(ctx, 1));
            const MbwEntry* ew = pick_mbw(d_dw->dtype, S, nrt, p.act_e == p.act_d ? p.act_e : -1, tw, kaw, rbw);
            if (!ew) return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: no kernel instantiation");
            return launch(ctx, mbw_kernel_of(*ew, nw, wl.total), gridw, (hipStream_t)stream, p);
        }
    }
    // block tiles (mbconv.hpp). Every unit that gets here has Cout <= 32: without a wave shape mbconv_unsupported admits no more, with
    // one the branch above is left only when mbw is switched off and block_shape holds (mbw_waves cannot return 0 for an admitted
    // unit: its window blocks are the same for both pixel-block widths, and mbconv_unsupported checked the 1 x 16 form). The kernel is
    // compiled for exactly that, so anything else is refused, not launched.
    if (p.nRowT != kMbRowT) return fail(ctx, PCV_ERR_INVALID, "pcv_mbconv_fused: unexpected packed layout");
    const MbLds lds = mbconv_plan(S, d_exp != nullptr, p.ka, p.nChunks, kMbRowT, &p.nbufX);
    const Kernel K = mbconv_kernel(d_dw->dtype, S, d_exp != nullptr, lds.total);
    int nb = 0;                 // (per launch: the resident blocks depend on the unit's LDS plan)
    if (int rc = blocks_per_cu(ctx, K, &nb)) return rc;
    const unsigned grid = (unsigned)std::min<long>(p.nTiles, (long)block_slots(ctx, nb));
    return launch(ctx, K, grid, (hipStream_t)stream, p);
}

int pcv_bn_act(pcv_ctx* ctx, const void* x, const float* scale, const float* shift, void* y, long rows, int C, int x_cpitch,
               int act, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (x_cpitch <= 0) x_cpitch = C;
    if (!x || !scale || !shift || !y || rows <= 0 || C <= 0 || C % 8 != 0 || x_cpitch < C || x_cpitch % 8 != 0 || !dtype_ok(dtype) ||
        act < 0 || act > PCV_ACT_HSWISH)
        return fail(ctx, PCV_ERR_INVALID, "pcv_bn_act: bad argument (C and x_cpitch must be multiples of 8, x_cpitch >= C)");
    const long total8 = rows * (C / 8);
    unsigned blocks = 0;
    if (int rc = stream_grid(ctx, "pcv_bn_act", total8, &blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    for_dtype(dtype, [&](auto T) { bn_act_kernel<DT_OF(T)><<<blocks, 256, 0, st>>>(x, scale, shift, y, total8, C, x_cpitch, act, ctx->ovf); });
    return launched(ctx);
}

int pcv_instnorm_workspace_bytes(int N, int Cn, size_t* bytes) {
    if (!bytes || N <= 0 || Cn < 0 || Cn % 8 != 0)
        return fail(nullptr, PCV_ERR_INVALID, "pcv_instnorm_workspace_bytes: bad argument (N > 0, Cn >= 0 and a multiple of 8)");
    *bytes = (size_t)N * (size_t)Cn * 2 * sizeof(float);
    return PCV_OK;
}

int pcv_instnorm_act(pcv_ctx* ctx, const void* x, const float* gamma, const float* beta, void* y, void* workspace, int N, int HW,
                     int C, int Cn, int x_cpitch, float eps, int act, int dtype, void* stream) {
    PCV_ENTER(ctx);
    if (x_cpitch <= 0) x_cpitch = C;
    if (!x || !y || N <= 0 || HW <= 0 || C <= 0 || Cn < 0 || Cn > C || C % 8 != 0 || Cn % 8 != 0 || x_cpitch < C || x_cpitch % 8 != 0 ||
        !(eps > 0.f) || !std::isfinite(eps) || !dtype_ok(dtype) || act < 0 || act > PCV_ACT_HSWISH)
        return fail(ctx, PCV_ERR_INVALID,
                    "pcv_instnorm_act: bad argument (N, HW, C > 0; 0 <= Cn <= C; C, Cn and x_cpitch multiples of 8; x_cpitch >= C; eps > 0)");
    if (Cn > 0 && (!gamma || !beta || !workspace || !aligned16(workspace)))
        return fail(ctx, PCV_ERR_INVALID, "pcv_instnorm_act: gamma, beta and a 16-byte aligned workspace are needed when Cn > 0");
    if (!in_window((unsigned long long)N * HW * x_cpitch * esize(dtype))) return too_large(ctx, "pcv_instnorm_act", "x");
    const long long bpi = ((long long)HW * (C / 8) + 255) / 256;          // apply: blocks per image, 256 chunks each
    unsigned blocks = 0;
    if (int rc = stream_grid(ctx, "pcv_instnorm_act", (long long)N * bpi * 256, &blocks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* ws = reinterpret_cast<float*>(workspace);
    if (Cn > 0) {
        const int groups = (Cn / 8 + kInGroup - 1) / kInGroup;
        const long long items = (long long)N * groups;          // < 2^31: N * Cn * 2 <= the bytes of x
        const unsigned sgrid = (unsigned)cap_blocks(ctx, items);
        for_dtype(dtype, [&](auto T) {
            instnorm_stats_kernel<DT_OF(T)><<<sgrid, kInThreads, 0, st>>>(x, gamma, beta, ws, HW, Cn, x_cpitch, eps, groups, (int)items);
        });
        if (int rc = launched(ctx)) return rc;
    }
    for_dtype(dtype, [&](auto T) {
        instnorm_apply_kernel<DT_OF(T)><<<blocks, 256, 0, st>>>(x, ws, y, (unsigned)(N * bpi), (unsigned)bpi, HW, C, Cn, x_cpitch, act, ctx->ovf);
    });
    return launched(ctx);
}

}  // extern "C"
