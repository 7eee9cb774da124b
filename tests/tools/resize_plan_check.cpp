// resize_plan_check.cpp - the host planner of the fused resize (pytorchcv_amd/csrc/resize_plan.hpp) as a stand-alone program, for a
// run under AddressSanitizer + UndefinedBehaviorSanitizer (tests/test_resize_host.py builds it with g++ -fsanitize=address,undefined
// and requires exit status 0). No HIP, no Python: it plans ragged batches - the ordinary ones, the extreme aspect ratios, the largest
// down-scales that are accepted and the ones that are refused - into exactly sized heap buffers, re-validates every blob the way the
// launch does and checks the invariants the kernel relies on for its bounds.
#include "resize_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace pcv_resize;

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                      \
        }                                                                    \
    } while (0)

struct Size { int h, w; };

// Plans the batch; when it is accepted, checks the blob. Returns whether it was accepted.
static bool plan_and_check(const std::vector<Size>& sizes, int C, int size, int H, int W) {
    const int N = (int)sizes.size();
    std::vector<int> hs, ws;
    std::vector<const void*> ptrs;
    for (int i = 0; i < N; ++i) {
        hs.push_back(sizes[i].h);
        ws.push_back(sizes[i].w);
        ptrs.push_back(reinterpret_cast<const void*>((uintptr_t)0x10000 * (i + 1)));
    }
    size_t bytes = 0;
    const char* why = plan_bytes(N, hs.data(), ws.data(), C, size, H, W, &bytes);
    if (why) {
        // the second call must refuse the same batch, whatever size it is told
        char dummy[16];
        CHECK(plan(ptrs.data(), N, hs.data(), ws.data(), C, size, H, W, dummy, sizeof(dummy)) != nullptr);
        return false;
    }
    char* blob = static_cast<char*>(std::malloc(bytes));        // exactly sized: a write past the end is the sanitizer's to find
    CHECK(blob != nullptr);
    CHECK(plan(ptrs.data(), N, hs.data(), ws.data(), C, size, H, W, blob, bytes + 16) != nullptr);
    CHECK(plan(ptrs.data(), N, hs.data(), ws.data(), C, size, H, W, blob, bytes) == nullptr);
    CHECK(validate(blob, bytes) == nullptr);
    CHECK(validate(blob, bytes - 1) != nullptr);
    ResizeHeader hd;
    std::memcpy(&hd, blob, sizeof(hd));
    CHECK(hd.N == N && hd.C == C && hd.H == H && hd.W == W && hd.bytes == bytes);
    const int pitch = stage_pitch(W, C);
    long long items = 0;
    for (int i = 0; i < N; ++i) {
        ResizeFrame g;
        std::memcpy(&g, blob + sizeof(hd) + (size_t)i * sizeof(g), sizeof(g));
        CHECK(g.Hs == sizes[i].h && g.Ws == sizes[i].w && g.top >= 0 && g.left >= 0 && g.top + H <= g.oh && g.left + W <= g.ow);
        const int32_t* ht = reinterpret_cast<const int32_t*>(blob + g.htab);
        const int32_t* vt = reinterpret_cast<const int32_t*>(blob + g.vtab);
        for (int x = 0; x < W; ++x) {
            long long sum = 0;
            CHECK(ht[x] >= 0 && ht[W + x] >= 1 && ht[W + x] <= g.hk && ht[x] + ht[W + x] <= g.Ws);
            for (int k = 0; k < g.hk; ++k) sum += ht[2 * W + (size_t)x * g.hk + k];
            CHECK(sum >= (1 << kPrecisionBits) - g.hk && sum <= (1 << kPrecisionBits) + g.hk);      // int32-safe times 255
        }
        for (int y = 0; y < H; ++y) {
            long long sum = 0;
            CHECK(vt[y] >= g.row0 && vt[H + y] >= 1 && vt[H + y] <= g.vk && vt[y] + vt[H + y] <= g.row1 && g.row1 <= g.Hs);
            if (y) CHECK(vt[y] >= vt[y - 1] && vt[y] + vt[H + y] >= vt[y - 1] + vt[H + y - 1]);       // windows move monotonically
            for (int k = 0; k < g.vk; ++k) sum += vt[2 * H + (size_t)y * g.vk + k];
            CHECK(sum >= (1 << kPrecisionBits) - g.vk && sum <= (1 << kPrecisionBits) + g.vk);
        }
        for (int y0 = 0; y0 < H; y0 += g.band) {
            const int yl = (y0 + g.band < H ? y0 + g.band : H) - 1;
            CHECK((long long)(vt[yl] + vt[H + yl] - vt[y0]) * pitch <= hd.stage_bytes);
        }
        CHECK(g.item0 == items);
        items += g.nbands;
    }
    CHECK(items == hd.items && hd.stage_bytes <= kStageBytes);
    // a corrupted header or frame is caught by the launch's validation
    std::vector<char> bad(blob, blob + bytes);
    bad[0] ^= 1;
    CHECK(validate(bad.data(), bytes) != nullptr);
    bad.assign(blob, blob + bytes);
    ResizeFrame g0;
    std::memcpy(&g0, bad.data() + sizeof(hd), sizeof(g0));
    g0.vtab = (uint32_t)bytes;
    std::memcpy(bad.data() + sizeof(hd), &g0, sizeof(g0));
    CHECK(validate(bad.data(), bytes) != nullptr);
    std::free(blob);
    return true;
}

int main() {
    const std::vector<Size> ragged = {{41, 53}, {53, 41}, {64, 64}, {7, 9}, {20, 25}, {37, 37}, {37, 64}, {300, 290}, {1000, 23}, {23, 1000}};
    for (int C = 1; C <= 4; ++C)
        for (int img : {32, 33, 40}) {
            const int size = img == 32 ? 37 : img == 33 ? 38 : 46;
            CHECK(plan_and_check(ragged, C, size, img, img));
        }
    CHECK(plan_and_check({{375, 500}, {500, 333}, {256, 256}, {2000, 3000}, {375, 500}, {256, 256}}, 3, 256, 224, 224));   // shared tables
    CHECK(plan_and_check({{1, 1}, {2, 3}, {4000, 4000}, {1, 4000}, {4000, 1}}, 1, 1, 1, 1));
    CHECK(plan_and_check({{4000, 4000}, {17, 17}}, 1, 341, 341, 341));
    CHECK(plan_and_check({{400000, 8}, {8, 400000}}, 3, 37, 32, 32));               // extreme aspect, both axes up-scale
    CHECK(plan_and_check({{12000, 12500}}, 3, 37, 32, 32));                         // the window of one row just fits: band 1
    CHECK(plan_and_check({{10000, 16000}}, 3, 256, 224, 224));                      // 39x down at the real crop size
    CHECK(!plan_and_check({{41, 53}, {400000, 400000}}, 3, 37, 32, 32));            // one-row window of 21,600 rows: refused
    CHECK(!plan_and_check({{20000, 21000}}, 3, 37, 32, 32));
    CHECK(!plan_and_check({{16000, 16000}}, 3, 256, 224, 224));
    CHECK(!plan_and_check({{16777216, 16777216}}, 1, 1, 1, 1));
    CHECK(!plan_and_check({{1, 16777216}}, 1, 37, 32, 32));                         // resized long side past the planner's limit
    CHECK(!plan_and_check({{41, 53}}, 5, 37, 32, 32));
    CHECK(!plan_and_check({{41, 53}}, 3, 37, 38, 32));
    CHECK(!plan_and_check({{41, 53}}, 3, 0, 32, 32));
    CHECK(!plan_and_check({{0, 53}}, 3, 37, 32, 32));
    CHECK(!plan_and_check({}, 3, 37, 32, 32));
    if (failures) std::fprintf(stderr, "%d check(s) failed\n", failures);
    else std::printf("resize planner: ok\n");
    return failures ? 1 : 0;
}
