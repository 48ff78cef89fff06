// CPU only: the host SIFT of sfm_features.hpp laid open for tests/test_sift_gpu.py -- the reference the device extractor is held to.
//   sift_ref <raw image> <rows> <cols> <channels> <out.bin> [max_features]
// raw image: rows * cols * channels bytes, dense (BGR where channels == 3).  out.bin, little endian:
//   int32 n_oct; per octave: int32 rows, cols, then the 6 Gaussian and the 5 DoG levels (float32, rows * cols each);
//   int32 n_ext, n_ext x {x, y, size, response} float32, n_ext x {octave, layer, r, c} int32: the extrema that pass adjust_extremum, before
//     orientation assignment, sorted by (octave, layer, r, c) of where the refinement ended;
//   int32 n_kp, n_kp x sfm_keypoint (28 B), n_kp x 128 float32: sift_detect_and_compute with nfeatures = max_features.
#include "../../sfm_opencv_amd/host/sfm_features.hpp"

#include <array>
#include <cstdlib>
#include <tuple>

using namespace sfm;

static void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("fwrite"); exit(2); } }
static void put_i32(FILE* f, int32_t v) { put(f, &v, 4); }

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: sift_ref <raw image> <rows> <cols> <channels> <out.bin> [max_features]\n"); return 1; }
    Image img;
    img.rows = atoi(argv[2]); img.cols = atoi(argv[3]); img.channels = atoi(argv[4]);
    img.data.resize((size_t)img.rows * img.cols * img.channels);
    FILE* in = fopen(argv[1], "rb");
    if (!in || fread(img.data.data(), 1, img.data.size(), in) != img.data.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    fclose(in);
    sift::Params P;
    P.nfeatures = argc > 6 ? atoi(argv[6]) : 0;
    FILE* f = fopen(argv[5], "wb");
    if (!f) { perror(argv[5]); return 1; }

    const sift::Pyramid py = sift::build_pyramid(sift::to_gray(img), P);
    put_i32(f, py.n_oct);
    for (int o = 0; o < py.n_oct; ++o) {
        put_i32(f, py.G(o, 0).rows); put_i32(f, py.G(o, 0).cols);
        for (int i = 0; i < P.layers + 3; ++i) put(f, py.G(o, i).v.data(), py.G(o, i).v.size() * 4);
        for (int i = 0; i < P.layers + 2; ++i) put(f, py.D(o, i).v.data(), py.D(o, i).v.size() * 4);
    }

    // the scan of sift_detect_and_compute up to adjust_extremum
    const float thr = (float)std::floor(0.5 * P.contrast / P.layers * 255.0);
    std::vector<std::pair<std::array<int, 4>, sift::Raw>> ext;
    for (int o = 0; o < py.n_oct; ++o)
        for (int i = 1; i <= P.layers; ++i) {
            const sift::Gray &pr = py.D(o, i - 1), &cu = py.D(o, i), &nx = py.D(o, i + 1);
            for (int r = 5; r < cu.rows - 5; ++r)
                for (int c = 5; c < cu.cols - 5; ++c) {
                    const float v = cu.at(r, c);
                    if (!(std::fabs(v) > thr)) continue;
                    bool e = true;
                    for (int dy = -1; dy <= 1 && e; ++dy)
                        for (int dx = -1; dx <= 1; ++dx) {
                            const float a = pr.at(r + dy, c + dx), b = nx.at(r + dy, c + dx), m = cu.at(r + dy, c + dx);
                            if (v > 0 ? (v < a || v < b || ((dx | dy) && v < m)) : (v > a || v > b || ((dx | dy) && v > m))) { e = false; break; }
                        }
                    if (!e) continue;
                    int layer = i, r1 = r, c1 = c;
                    sift::Raw kp;
                    if (!sift::adjust_extremum(py, P, o, layer, r1, c1, kp)) continue;
                    ext.push_back({ { o, layer, r1, c1 }, kp });
                }
        }
    std::stable_sort(ext.begin(), ext.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    put_i32(f, (int32_t)ext.size());
    for (const auto& e : ext) { const float v[4] = { e.second.x, e.second.y, e.second.size, e.second.response }; put(f, v, 16); }
    for (const auto& e : ext) { const int32_t v[4] = { e.first[0], e.first[1], e.first[2], e.first[3] }; put(f, v, 16); }

    std::vector<KeyPoint> kps;
    Mat desc;
    sift_detect_and_compute(img, kps, desc, P);
    put_i32(f, (int32_t)kps.size());
    for (const KeyPoint& k : kps) {
        sfm_keypoint q;
        q.x = k.pt.x; q.y = k.pt.y; q.size = k.size; q.angle = k.angle; q.response = k.response; q.octave = k.octave; q.class_id = k.class_id;
        put(f, &q, sizeof q);
    }
    for (int i = 0; i < (int)kps.size(); ++i) put(f, desc.ptr<float>(i), 128 * 4);
    fclose(f);
    return 0;
}
