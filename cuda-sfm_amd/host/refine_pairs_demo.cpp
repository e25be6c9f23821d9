// refine_pairs_demo.cpp -- many view pairs refined in one batched call (SfM::refine_pairs of sfm.h, sfm_refine_pairs):
//   per pair: features -> MatchSiftData -> SfM::Image_pair -> fillXU -> estimateE; then ONE refine_pairs over all of them.
// The feature sets come from files of raw SiftPoint records (as two_view_demo reads them), two per pair:
//     refine_pairs_demo <refine_iterations> <a1.bin> <a2.bin> [<b1.bin> <b2.bin> ...]
// One line per pair, in sfm_main's format: what sfm_main prints for that pair alone (same camera, same estimateE settings).
// Plain C++: needs only the facade headers and libsfm_amd.so.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "sfm.h"
#include "sfm_io.h"

static std::vector<SiftPoint> read_sift(const char *path)
{
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<SiftPoint> v((size_t)bytes / sizeof(SiftPoint));
    if (!v.empty() && std::fread(v.data(), sizeof(SiftPoint), v.size(), f) != v.size()) { std::perror("fread"); std::exit(2); }
    std::fclose(f);
    return v;
}

static void upload(SiftData &data, const char *path)
{
    const std::vector<SiftPoint> f = read_sift(path);
    InitSiftData(data, 32768, true, true);
    if (f.size() > 32768) { std::fprintf(stderr, "%s: more than 32768 records\n", path); std::exit(2); }
    data.numPts = (int)f.size();
    std::copy(f.begin(), f.end(), data.h_data);
    UploadSiftData(data);                                   // stands in for ExtractSift
}

int main(int argc, char **argv)
{
    if (argc < 4 || (argc - 2) % 2 != 0) {
        std::fprintf(stderr, "usage: %s refine_iterations a1.bin a2.bin [b1.bin b2.bin ...]\n", argv[0]);
        return 2;
    }
    const int iterations = std::atoi(argv[1]), count = (argc - 2) / 2;
    const unsigned w = 720, h = 576;                        // dino frames (main.cpp:254-256)
    float K[9] = { 2360.0f, 0, (float)(w / 2.0), 0, 2360, (float)(h / 2.0), 0, 0, 1 };       // main.cpp:292-297
    float inv_K[9] = { (float)(1.0 / 2360), 0, (float)(-(w / 2.0) / 2360), 0, (float)(1.0 / 2360), (float)(-(h / 2.0) / 2360), 0, 0, 1 };

    InitCuda(0);
    std::vector<SiftData> sift((size_t)2 * count);
    std::vector<std::unique_ptr<SfM::Image_pair>> owned;
    std::vector<SfM::Image_pair *> pairs;
    for (int k = 0; k < count; ++k) {
        SiftData &s1 = sift[(size_t)2 * k], &s2 = sift[(size_t)2 * k + 1];
        upload(s1, argv[2 + 2 * k]);
        upload(s2, argv[3 + 2 * k]);
        MatchSiftData(s1, s2);
        owned.emplace_back(new SfM::Image_pair(K, inv_K, 2, s1.numPts));
        owned.back()->fillXU(s1.d_data);
        owned.back()->estimateE();
        pairs.push_back(owned.back().get());
    }
    const std::vector<sfm_refine_report> reports = SfM::refine_pairs(pairs.data(), count, iterations);
    for (const sfm_refine_report &rep : reports)
        std::printf("refine: %d points, rms %.4f -> %.4f px, %d iterations\n", rep.num_used, rep.initial_rms_px, rep.final_rms_px, rep.iterations);
    owned.clear();
    for (SiftData &s : sift) FreeSiftData(s);
    return 0;
}
