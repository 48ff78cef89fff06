// CPU only: the host AKAZE of sfm_akaze.hpp laid open for tests/test_akaze_gpu.py and tests/test_akaze_cpu.py -- the reference the
// device extractor is held to.
//   akaze_ref <raw image> <rows> <cols> <channels> <out.bin> [max_features]
// raw image: rows * cols * channels bytes, dense (BGR where channels == 3).  out.bin, little endian:
//   int32 n_levels; per level: int32 rows, cols, float32 kcontrast (the factor its diffusion used; level 0: k_percentile's result), then
//     Lt, Lsmooth, Lx, Ly, Ldet (float32, rows * cols each);
//   three lists, each int32 n, n x {x, y, size, response} float32, n x {octave, level} int32:
//     the raw 3 x 3 maxima in find_extrema's scan order (restated here: its two conditions, without the suppression),
//     find_extrema's result, and what subpixel keeps of it;
//   int32 n_kp, n_kp x sfm_keypoint (28 B), n_kp x 61 bytes: akaze_detect_and_compute with max_features.
#include "../../sfm_opencv_amd/host/sfm_features.hpp"

#include <cstdlib>

using namespace sfm;

static void put(FILE* f, const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) { perror("fwrite"); exit(2); } }
static void put_i32(FILE* f, int32_t v) { put(f, &v, 4); }
static void put_list(FILE* f, const std::vector<akaze::Cand>& v)
{
    put_i32(f, (int32_t)v.size());
    for (const auto& c : v) { const float q[4] = { c.x, c.y, c.size, c.response }; put(f, q, 16); }
    for (const auto& c : v) { const int32_t q[2] = { c.octave, c.level }; put(f, q, 8); }
}

int main(int argc, char** argv)
{
    if (argc < 6) { fprintf(stderr, "usage: akaze_ref <raw image> <rows> <cols> <channels> <out.bin> [max_features]\n"); return 1; }
    Image img;
    img.rows = atoi(argv[2]); img.cols = atoi(argv[3]); img.channels = atoi(argv[4]);
    img.data.resize((size_t)img.rows * img.cols * img.channels);
    FILE* in = fopen(argv[1], "rb");
    if (!in || fread(img.data.data(), 1, img.data.size(), in) != img.data.size()) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    fclose(in);
    const int max_features = argc > 6 ? atoi(argv[6]) : 0;
    FILE* f = fopen(argv[5], "wb");
    if (!f) { perror(argv[5]); return 1; }

    const akaze::Params P;
    sift::Gray g = sift::to_gray(img);
    for (float& v : g.v) v *= 1.0f / 255.0f;
    const std::vector<akaze::Level> ev = akaze::build_scale_space(g, P);
    put_i32(f, (int32_t)ev.size());
    float kcontrast = ev.empty() ? 0.0f : akaze::k_percentile(g, P);
    for (size_t i = 0; i < ev.size(); ++i) {
        if (i > 0 && ev[i].octave > ev[i - 1].octave) kcontrast *= 0.75f;
        put_i32(f, ev[i].Lt.rows); put_i32(f, ev[i].Lt.cols); put(f, &kcontrast, 4);
        for (const sift::Gray* a : { &ev[i].Lt, &ev[i].Lsmooth, &ev[i].Lx, &ev[i].Ly, &ev[i].Ldet }) put(f, a->v.data(), a->v.size() * 4);
    }

    // the scan of find_extrema without its suppression
    std::vector<akaze::Cand> raw;
    const float smax = 12.0f * std::sqrt(2.0f);
    for (size_t i = 0; i < ev.size(); ++i) {
        const akaze::Level& L = ev[i];
        const float ratio = (float)(1 << L.octave);
        const int border = akaze::fround(smax * L.sigma_size) + 1;
        for (int y = border; y < L.Ldet.rows - border; ++y)
            for (int x = border; x < L.Ldet.cols - border; ++x) {
                const float v = L.Ldet.at(y, x);
                if (!(v > P.dthreshold)) continue;
                if (!(v > L.Ldet.at(y, x - 1) && v > L.Ldet.at(y, x + 1) && v > L.Ldet.at(y - 1, x - 1) && v > L.Ldet.at(y - 1, x) && v > L.Ldet.at(y - 1, x + 1) &&
                      v > L.Ldet.at(y + 1, x - 1) && v > L.Ldet.at(y + 1, x) && v > L.Ldet.at(y + 1, x + 1))) continue;
                raw.push_back(akaze::Cand{ x * ratio, y * ratio, L.esigma * P.derivative_factor, v, L.octave, (int)i });
            }
    }
    put_list(f, raw);
    const std::vector<akaze::Cand> cand = akaze::find_extrema(ev, P);
    put_list(f, cand);
    std::vector<akaze::Cand> kept;
    for (akaze::Cand c : cand) if (akaze::subpixel(ev, c)) kept.push_back(c);
    put_list(f, kept);

    std::vector<KeyPoint> kps;
    Mat desc;
    akaze_detect_and_compute(img, kps, desc, max_features);
    put_i32(f, (int32_t)kps.size());
    for (const KeyPoint& k : kps) {
        sfm_keypoint q;
        q.x = k.pt.x; q.y = k.pt.y; q.size = k.size; q.angle = k.angle; q.response = k.response; q.octave = k.octave; q.class_id = k.class_id;
        put(f, &q, sizeof q);
    }
    for (int i = 0; i < (int)kps.size(); ++i) put(f, desc.ptr<uint8_t>(i), 61);
    fclose(f);
    return 0;
}
