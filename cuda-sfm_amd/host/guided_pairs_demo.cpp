// guided_pairs_demo.cpp -- the guided second matching pass of MANY pairs in one batched call (MatchSiftDataGuidedPairs of
// cudaSift.h, SfM::refine_pairs and SfM::fundamentals of sfm.h; sfm_match_guided_pairs):
//   per pair: features -> MatchSiftData -> SfM::Image_pair -> fillXU -> estimateE;
//   then ONE refine_pairs, ONE fundamentals and ONE MatchSiftDataGuidedPairs over all of them.
// The feature sets come from files of raw SiftPoint records (as guided_match_demo reads them), first views first:
//     guided_pairs_demo <k> <a1.bin> .. <ak.bin> <b1.bin> .. <bk.bin> [band_px]
// Pair i is (a_i, b_i); every pair loads its own copy of its records, so two pairs may name the same file.  It prints one
// "plain:" and one "guided:" line per pair in guided_match_demo's format.  Plain C++: needs only the facade headers and
// libsfm_amd.so.
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
    const int count = argc > 1 ? std::atoi(argv[1]) : 0;
    if (count < 1 || (argc != 2 + 2 * count && argc != 3 + 2 * count)) {
        std::fprintf(stderr, "usage: %s k a1.bin .. ak.bin b1.bin .. bk.bin [band_px]\n", argv[0]);
        return 2;
    }
    const float band = argc == 3 + 2 * count ? (float)std::atof(argv[2 + 2 * count]) : 4.0f;
    const unsigned w = 720, h = 576;                        // dino frames (main.cpp:254-256)
    float K[9] = { 2360.0f, 0, (float)(w / 2.0), 0, 2360, (float)(h / 2.0), 0, 0, 1 };       // main.cpp:292-297
    float inv_K[9] = { (float)(1.0 / 2360), 0, (float)(-(w / 2.0) / 2360), 0, (float)(1.0 / 2360), (float)(-(h / 2.0) / 2360), 0, 0, 1 };

    InitCuda(0);
    std::vector<SiftData> first((size_t)count), second((size_t)count);
    std::vector<SiftData *> p1, p2;
    std::vector<std::unique_ptr<SfM::Image_pair>> owned;
    std::vector<SfM::Image_pair *> pairs;
    for (int k = 0; k < count; ++k) {
        SiftData &s1 = first[(size_t)k], &s2 = second[(size_t)k];
        upload(s1, argv[2 + k]);
        upload(s2, argv[2 + count + k]);
        if (!s1.numPts || !s2.numPts) { std::fprintf(stderr, "pair %d: an empty feature file\n", k); return 2; }
        MatchSiftData(s1, s2);
        print_line("plain:", s1);
        owned.emplace_back(new SfM::Image_pair(K, inv_K, 2, s1.numPts));
        owned.back()->fillXU(s1.d_data);
        owned.back()->estimateE();
        pairs.push_back(owned.back().get());
        p1.push_back(&s1);
        p2.push_back(&s2);
    }
    const std::vector<sfm_refine_report> reports = SfM::refine_pairs(pairs.data(), count, 20);
    for (const sfm_refine_report &rep : reports)
        std::printf("refine: %d points, rms %.4f -> %.4f px, %d iterations\n", rep.num_used, rep.initial_rms_px, rep.final_rms_px, rep.iterations);
    {
        const std::shared_ptr<float> F = SfM::fundamentals(pairs.data(), count, true);
        MatchSiftDataGuidedPairs(p1.data(), p2.data(), F.get(), count, band);      // (the copies back to the hosts wait for it)
    }
    for (int k = 0; k < count; ++k) print_line("guided:", first[(size_t)k]);
    owned.clear();
    for (SiftData &s : first) FreeSiftData(s);
    for (SiftData &s : second) FreeSiftData(s);
    return 0;
}
