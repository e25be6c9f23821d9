// register_views_demo.cpp -- a third view registered to each of many view pairs in one batched call (SfM::register_views of
// sfm.h, sfm_register_views):
//   per triple: features -> MatchSiftData(1, 2) -> SfM::Image_pair -> fillXU -> estimateE; then ONE refine_pairs over all pairs;
//   then MatchSiftData(1, 3) per triple and ONE register_views over all of them.
// The feature sets come from files of raw SiftPoint records (as two_view_demo reads them), three per triple:
//     register_views_demo <refine_iterations> <a1.bin> <a2.bin> <a3.bin> [<b1.bin> <b2.bin> <b3.bin> ...]
//   then ONE triangulate_views over all of them: every pair's points over its three views.
//   then ONE adjust_views over all of them (both cameras and the points over the three views), and per triple one more
//   triangulateView with its adjusted cameras.
// Four lines per triple: the view3, view3 points, adjust and adjusted view3 points lines sfm_main prints for that triple alone
// (same camera, same settings, the same refine_iterations).
// Plain C++: needs only the facade headers and libsfm_amd.so.
#include <algorithm>
#include <cmath>
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
    if (argc < 5 || (argc - 2) % 3 != 0) {
        std::fprintf(stderr, "usage: %s refine_iterations a1.bin a2.bin a3.bin [b1.bin b2.bin b3.bin ...]\n", argv[0]);
        return 2;
    }
    const int iterations = std::atoi(argv[1]), count = (argc - 2) / 3;
    const unsigned w = 720, h = 576;                        // dino frames (main.cpp:254-256)
    float K[9] = { 2360.0f, 0, (float)(w / 2.0), 0, 2360, (float)(h / 2.0), 0, 0, 1 };       // main.cpp:292-297
    float inv_K[9] = { (float)(1.0 / 2360), 0, (float)(-(w / 2.0) / 2360), 0, (float)(1.0 / 2360), (float)(-(h / 2.0) / 2360), 0, 0, 1 };

    InitCuda(0);
    std::vector<SiftData> sift((size_t)3 * count);
    std::vector<std::unique_ptr<SfM::Image_pair>> owned;
    std::vector<SfM::Image_pair *> pairs;
    for (int k = 0; k < count; ++k) {
        SiftData &s1 = sift[(size_t)3 * k], &s2 = sift[(size_t)3 * k + 1], &s3 = sift[(size_t)3 * k + 2];
        upload(s1, argv[2 + 3 * k]);
        upload(s2, argv[3 + 3 * k]);
        upload(s3, argv[4 + 3 * k]);
        MatchSiftData(s1, s2);
        owned.emplace_back(new SfM::Image_pair(K, inv_K, 2, s1.numPts));
        owned.back()->fillXU(s1.d_data);
        owned.back()->estimateE();
        pairs.push_back(owned.back().get());
    }
    SfM::refine_pairs(pairs.data(), count, iterations);
    std::vector<SiftPoint *> records;
    for (int k = 0; k < count; ++k) {
        MatchSiftData(sift[(size_t)3 * k], sift[(size_t)3 * k + 2]);                // rewrites view 1's match fields only
        records.push_back(sift[(size_t)3 * k].d_data);
    }
    const std::vector<sfm_register_report> reports = SfM::register_views(pairs.data(), records.data(), count);
    const std::vector<SfM::ViewPoints> clouds = SfM::triangulate_views(pairs.data(), records.data(), count);
    const std::vector<SfM::ViewAdjust> adjusted = SfM::adjust_views(pairs.data(), records.data(), clouds.data(), count);
    for (int k = 0; k < count; ++k) {
        const sfm_register_report &vr = reports[(size_t)k];
        float P3[16];
        pairs[(size_t)k]->getViewPose(P3);
        double nc = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double c = -((double)P3[a] * P3[3] + (double)P3[4 + a] * P3[7] + (double)P3[8 + a] * P3[11]);
            nc += c * c;
        }
        std::printf("view3: %d/%d inliers, rms %.4f -> %.4f px, |C3| %.4f\n", vr.num_inliers, vr.num_candidates, vr.initial_rms_px,
                    vr.final_rms_px, std::sqrt(nc));
        const int32_t *c = clouds[(size_t)k].counts;
        std::printf("view3 points: %d new, %d refined, %d kept, %d rejected\n", c[SFM_VP_NEW], c[SFM_VP_REFINED], c[SFM_VP_KEPT], c[SFM_VP_NEW_REJECTED]);
        const SfM::ViewAdjust &adj = adjusted[(size_t)k];
        std::printf("adjust: %d points (%d / %d in views 2 / 3), rms %.4f -> %.4f px, %d iterations\n", adj.report.num_points, adj.report.num_view2,
                    adj.report.num_view3, adj.report.initial_rms_px, adj.report.final_rms_px, adj.report.iterations);
        const SfM::ViewPoints again = pairs[(size_t)k]->triangulateView(records[(size_t)k], 5, 4.0f, 1.0f, adj.poses);
        std::printf("adjusted view3 points: %d new, %d refined, %d kept, %d rejected\n", again.counts[SFM_VP_NEW], again.counts[SFM_VP_REFINED],
                    again.counts[SFM_VP_KEPT], again.counts[SFM_VP_NEW_REJECTED]);
    }
    owned.clear();
    for (SiftData &s : sift) FreeSiftData(s);
    return 0;
}
