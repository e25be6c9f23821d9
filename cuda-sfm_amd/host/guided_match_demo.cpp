// guided_match_demo.cpp -- a second, guided matching pass once the pair's geometry is known (MatchSiftDataGuided of cudaSift.h,
// SfM::Image_pair::fundamental of sfm.h; sfm_match_guided, sfm_pair_fundamental):
//   features -> MatchSiftData -> SfM::Image_pair -> fillXU -> estimateE -> refine -> fundamental(true) -> MatchSiftDataGuided.
// The feature sets come from two files of raw SiftPoint records (as two_view_demo reads them):
//     guided_match_demo <a1.bin> <a2.bin> [band_px]
// It prints one "plain:" and one "guided:" line, each with the number of records of the first set that pass the gates the later
// stages apply (score > 0.85, ambiguity < 0.95).  Plain C++: needs only the facade headers and libsfm_amd.so.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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

static void print_line(const char *label, const SiftData &d)
{
    int matched = 0, accepted = 0;
    for (int i = 0; i < d.numPts; ++i) {
        const SiftPoint &p = d.h_data[i];
        matched += p.match >= 0;
        accepted += p.match >= 0 && p.score > 0.85f && p.ambiguity < 0.95f;
    }
    std::printf("%s %d records, %d matched, %d pass 0.85 / 0.95\n", label, d.numPts, matched, accepted);
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc > 4) {
        std::fprintf(stderr, "usage: %s a1.bin a2.bin [band_px]\n", argv[0]);
        return 2;
    }
    const float band = argc > 3 ? (float)std::atof(argv[3]) : 4.0f;
    const unsigned w = 720, h = 576;                        // dino frames (main.cpp:254-256)
    float K[9] = { 2360.0f, 0, (float)(w / 2.0), 0, 2360, (float)(h / 2.0), 0, 0, 1 };       // main.cpp:292-297
    float inv_K[9] = { (float)(1.0 / 2360), 0, (float)(-(w / 2.0) / 2360), 0, (float)(1.0 / 2360), (float)(-(h / 2.0) / 2360), 0, 0, 1 };

    InitCuda(0);
    SiftData s1, s2;
    upload(s1, argv[1]);
    upload(s2, argv[2]);
    if (!s1.numPts || !s2.numPts) { std::fprintf(stderr, "an empty feature file\n"); return 2; }
    MatchSiftData(s1, s2);
    print_line("plain:", s1);
    {
        SfM::Image_pair pair(K, inv_K, 2, s1.numPts);
        pair.fillXU(s1.d_data);
        pair.estimateE();
        const sfm_refine_report rep = pair.refine(20);
        std::printf("refine: %d points, rms %.4f -> %.4f px, %d iterations\n", rep.num_used, rep.initial_rms_px, rep.final_rms_px, rep.iterations);
        MatchSiftDataGuided(s1, s2, pair.fundamental(true), band);
    }
    print_line("guided:", s1);
    FreeSiftData(s1);
    FreeSiftData(s2);
    return 0;
}
