// mb_lds_check.cpp - host-only: prints the LDS totals of the three fused inverted-residual kernels' layout functions (csrc/mbr.hpp,
// csrc/mbw.hpp, csrc/mbconv.hpp) for the argument rows of a text file, one total per row, for tests/test_mbconv_ref_bounds.py to
// compare with its Python restatement. No device is touched.
//   mbr nrt nChunks ka afl wel xrows waves | mbw stride nrt nChunks nWaves tw ka rb | mb stride expand ka nChunks nRowT nbufX
#include <cstdio>
#include <cstring>
#include "mbconv.hpp"      // (each includes csrc/mb_device.hpp and no sibling: any order, any subset)
#include "mbw.hpp"
#include "mbr.hpp"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    char kind[8];
    int a[7];
    while (std::fscanf(f, "%7s %d %d %d %d %d %d", kind, &a[0], &a[1], &a[2], &a[3], &a[4], &a[5]) == 7) {
        if (!std::strcmp(kind, "mb")) {
            std::printf("%d\n", mb_lds_layout(a[0], a[1] != 0, a[2], a[3], a[4], a[5]).total);
            continue;
        }
        if (std::fscanf(f, "%d", &a[6]) != 1) return 3;
        if (!std::strcmp(kind, "mbr")) std::printf("%d\n", mbr_lds_layout(a[0], a[1], a[2], a[3] != 0, a[4] != 0, a[5], a[6]).total);
        else if (!std::strcmp(kind, "mbw")) std::printf("%d\n", mbw_lds_layout(a[0], a[1], a[2], a[3], a[4], a[5], a[6]).total);
        else return 3;
    }
    std::fclose(f);
    return 0;
}
