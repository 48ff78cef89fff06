// jpeg_scan_test -- the two halves decode_jpeg is made of (sfm_jpeg.hpp: parse_headers, decode_scan) with a coefficient sink, the way
// the device decoder's host entropy path uses them.  Host code only; built with AddressSanitizer + UBSan by tests/host/jpeg_scan.mk.
//
//   jpeg_scan_test FILE...
//
// One line per file: "FILE refused-headers", "FILE refused-scan" or "FILE ok rows cols channels restart intervals blocks...".  For an
// accepted file every component must have received blocks x 64 coefficients, every block exactly once and inside the padded plane, and
// decode_jpeg must accept it too.  Exit status 0 when that holds for every file, 2 otherwise.
#include <cstdio>
#include <fstream>
#include <vector>

#include "sfm_jpeg.hpp"

int main(int argc, char** argv)
{
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream f(argv[a], std::ios::binary);
        std::vector<uint8_t> d((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        sfm::jpeg::Frame fr;
        int rows = 0, cols = 0, ch = 0; std::vector<uint8_t> px;
        const bool whole = sfm::jpeg::decode_jpeg(d.data(), d.size(), rows, cols, ch, px);
        if (!sfm::jpeg::parse_headers(d.data(), d.size(), fr)) {
            printf("%s refused-headers\n", argv[a]);
            if (whole) { printf("  decode_jpeg accepted it\n"); bad = 1; }
            continue;
        }
        std::vector<std::vector<int16_t>> coef(fr.comp.size());
        std::vector<std::vector<uint8_t>> seen(fr.comp.size());
        std::vector<size_t> count(fr.comp.size(), 0);
        for (size_t c = 0; c < fr.comp.size(); ++c) {
            const size_t blocks = (size_t)(fr.comp[c].pw / 8) * (fr.comp[c].ph / 8);
            coef[c].assign(blocks * 64, 0); seen[c].assign(blocks, 0);
        }
        bool inside = true;
        const bool ok = sfm::jpeg::decode_scan(d.data(), d.size(), fr, [&](int ci, int brow, int bcol, const int* qc) {
            const sfm::jpeg::Component& c = fr.comp[(size_t)ci];
            if (brow < 0 || bcol < 0 || brow >= c.ph / 8 || bcol >= c.pw / 8) { inside = false; return; }
            const size_t b = (size_t)brow * (c.pw / 8) + bcol;
            if (seen[(size_t)ci][b]++) inside = false;
            for (int z = 0; z < 64; ++z) {
                if (qc[z] < -32768 || qc[z] > 32767) inside = false;          // the int16 layout holds every value
                coef[(size_t)ci][b * 64 + z] = (int16_t)qc[z];
            }
            count[(size_t)ci] += 64;
        });
        if (!inside) { printf("%s a block outside its plane, twice, or a value outside 16 bits\n", argv[a]); bad = 1; }
        if (ok != whole) { printf("%s decode_scan %d, decode_jpeg %d\n", argv[a], (int)ok, (int)whole); bad = 1; }
        if (!ok) { printf("%s refused-scan\n", argv[a]); continue; }
        printf("%s ok %d %d %d %d %lld", argv[a], fr.H, fr.W, fr.comp.size() == 1 ? 1 : 3, fr.restart, fr.intervals());
        for (size_t c = 0; c < fr.comp.size(); ++c) {
            printf(" %zu", seen[c].size());
            if (count[c] != seen[c].size() * 64) bad = 1;
        }
        if (rows != fr.H || cols != fr.W) bad = 1;
        printf("\n");
    }
    return bad ? 2 : 0;
}
