// align_pairs_demo.cpp -- a chain of overlapping view pairs put into one frame (SfM::align_pairs of sfm.h, sfm_align_pairs):
//   per pair: features -> MatchSiftData -> SfM::Image_pair -> fillXU -> estimateE; ONE refine_pairs over all of them; ONE
//   align_pairs over the k - 1 links (pair i -> pair i + 1); the links composed into every pair's transform to pair 1's frame.
// The feature sets come from files of raw SiftPoint records (as refine_pairs_demo reads them):
//     align_pairs_demo <k> <a1.bin> .. <ak.bin> <b1.bin> .. <bk.bin> [cloud.ply]
// a_i / b_i: the records of pair i's first / second view.  Pair i + 1's first view is pair i's second: a_{i+1} must hold the
// records of b_i's view (same count, same positions), or the program refuses -- a record's match index is the next pair's point.
// One line per link, then the cloud of all pairs' used refined points in pair 1's frame as a PLY (default chained_cloud.ply).
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

static void upload(SiftData &data, const std::vector<SiftPoint> &f, const char *path)
{
    InitSiftData(data, 32768, true, true);
    if (f.size() > 32768) { std::fprintf(stderr, "%s: more than 32768 records\n", path); std::exit(2); }
    data.numPts = (int)f.size();
    std::copy(f.begin(), f.end(), data.h_data);
    UploadSiftData(data);                                   // stands in for ExtractSift
}

int main(int argc, char **argv)
{
    const int count = argc > 1 ? std::atoi(argv[1]) : 0;
    if (count < 2 || (argc != 2 + 2 * count && argc != 3 + 2 * count)) {
        std::fprintf(stderr, "usage: %s k a1.bin .. ak.bin b1.bin .. bk.bin [cloud.ply]   (k >= 2)\n", argv[0]);
        return 2;
    }
    const char *ply = argc == 3 + 2 * count ? argv[2 + 2 * count] : "chained_cloud.ply";
    const unsigned w = 720, h = 576;                        // dino frames (main.cpp:254-256)
    float K[9] = { 2360.0f, 0, (float)(w / 2.0), 0, 2360, (float)(h / 2.0), 0, 0, 1 };       // main.cpp:292-297
    float inv_K[9] = { (float)(1.0 / 2360), 0, (float)(-(w / 2.0) / 2360), 0, (float)(1.0 / 2360), (float)(-(h / 2.0) / 2360), 0, 0, 1 };

    std::vector<std::vector<SiftPoint>> fa, fb;
    for (int k = 0; k < count; ++k) { fa.push_back(read_sift(argv[2 + k])); fb.push_back(read_sift(argv[2 + count + k])); }
    for (int k = 0; k + 1 < count; ++k) {                   // the link's correspondence: b_k and a_{k+1} are one view's records
        const std::vector<SiftPoint> &x = fb[(size_t)k], &y = fa[(size_t)k + 1];
        bool same = x.size() == y.size();
        for (size_t j = 0; same && j < x.size(); ++j) same = x[j].xpos == y[j].xpos && x[j].ypos == y[j].ypos;
        if (!same) {
            std::fprintf(stderr, "%s and %s are not the records of one view (count or positions differ)\n", argv[2 + count + k], argv[3 + k]);
            return 2;
        }
    }

    InitCuda(0);
    std::vector<SiftData> sift((size_t)2 * count);
    std::vector<std::unique_ptr<SfM::Image_pair>> owned;
    std::vector<SfM::Image_pair *> pairs;
    std::vector<SiftPoint *> records;
    for (int k = 0; k < count; ++k) {
        SiftData &s1 = sift[(size_t)2 * k], &s2 = sift[(size_t)2 * k + 1];
        upload(s1, fa[(size_t)k], argv[2 + k]);
        upload(s2, fb[(size_t)k], argv[2 + count + k]);
        MatchSiftData(s1, s2);
        owned.emplace_back(new SfM::Image_pair(K, inv_K, 2, s1.numPts));
        owned.back()->fillXU(s1.d_data);
        owned.back()->estimateE();
        pairs.push_back(owned.back().get());
        records.push_back(s1.d_data);
    }
    SfM::refine_pairs(pairs.data(), count);
    const std::vector<SfM::PairLink> links = SfM::align_pairs(pairs.data(), pairs.data() + 1, records.data(), count - 1);
    for (const SfM::PairLink &l : links)
        std::printf("align: %d candidates, %d inliers, s %.5f, rms %.4f -> %.4f px, %d iterations\n", l.report.num_candidates, l.report.num_inliers,
                    l.sim.s, l.report.initial_rms_px, l.report.final_rms_px, l.report.iterations);

    // every pair's used refined points in pair 1's frame: the inverse links composed along the chain
    std::vector<float> cloud;                               // x, y, z per point
    SfM::Sim3 to_first;                                     // pair k -> pair 1
    for (int k = 0; k < count; ++k) {
        if (k > 0) to_first = to_first.compose(links[(size_t)k - 1].sim.inverse());
        const int n = pairs[(size_t)k]->numPoints();
        std::vector<uint8_t> used;
        pairs[(size_t)k]->getReprojectionErrors(&used);
        const std::vector<float> pts = pairs[(size_t)k]->getRefinedPoints();
        for (int j = 0; j < n; ++j) {
            if (!used[(size_t)j]) continue;
            const double W = pts[(size_t)3 * n + j];
            const double X[3] = { pts[(size_t)j] / W, pts[(size_t)n + j] / W, pts[(size_t)2 * n + j] / W };
            double Y[3];
            to_first.apply(X, Y);
            for (int c = 0; c < 3; ++c) cloud.push_back((float)Y[c]);
        }
    }
    const int total = (int)(cloud.size() / 3);
    std::vector<float> cols((size_t)4 * total, 1.0f);       // WritePLY's 4 x N layout
    for (int j = 0; j < total; ++j)
        for (int c = 0; c < 3; ++c) cols[(size_t)c * total + j] = cloud[(size_t)3 * j + c];
    const int written = WritePLY(ply, cols.data(), total);
    std::printf("chained cloud: %d points -> %s\n", written, ply);
    owned.clear();
    for (SiftData &s : sift) FreeSiftData(s);
    return 0;
}
