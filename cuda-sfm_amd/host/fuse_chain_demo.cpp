// fuse_chain_demo.cpp -- a chain of overlapping view pairs fused into tracks and one point per track (SfM::fuse_chain of sfm.h:
// sfm_align_pairs, then sfm_fuse_chain):
//   per pair: features -> MatchSiftData -> SfM::Image_pair -> fillXU -> estimateE; ONE refine_pairs over all of them; ONE
//   fuse_chain over the chain (pair i -> pair i + 1).
// The arguments are align_pairs_demo's:
//     fuse_chain_demo <k> <a1.bin> .. <ak.bin> <b1.bin> .. <bk.bin> [cloud.ply [adjust_iterations [ring | loop]]]
// a_i / b_i: files of raw SiftPoint records of pair i's first / second view; a_{i+1} must hold the records of b_i's view.
// With the word `ring` behind adjust_iterations the pairs are a ring (k >= 3, b_k holds the records of a_1's view): pair k is also
// aligned onto pair 1, SfM::close_ring spreads the drift over the k links, one `ring:` line is printed first and the chain is
// fused over the corrected links.  Without it nothing changes.  With the word `loop` in its place the ring is closed in the same
// way and then fused as a RING by SfM::fuse_ring over all k corrected links: the tracks that cross the seam are joined, and one
// `seam:` line follows the `fuse:` line (status, closure, proposals, seam tracks refined / kept).
// One `fuse:` line, then the fused cloud of the first segment -- one point per track, where align_pairs_demo writes a feature
// once per pair that sees it -- as a PLY (default fused_cloud.ply).  With adjust_iterations > 0 (default 0: nothing changes) one
// SfM::adjust_chain over the fused model follows, one `chain adjust:` line per segment is printed and the PLY holds the adjusted
// points.  With `loop`, adjust_iterations > 0 and a ring that closed, SfM::adjust_ring follows as well (one camera per view, the
// seam tracks used): one `ring adjust:` line behind the `chain adjust:` lines, and the PLY holds ITS points.
// An adjustment moves every camera and rewrites only the tracks it used, so behind the last adjustment SfM::intersect_tracks brings
// every other track (kept, over-long, seam tracks of a plain chain adjustment) under the adjusted cameras, the used ones skipped:
// one `intersect:` line with its eight counts -- on stderr: stdout keeps exactly the lines it had with an adjustment -- and the PLY
// holds its points.  Without an adjustment there is no such line and nothing changes.
// Plain C++: needs only the facade headers and libsfm_amd.so.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>
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
    const bool loop = count >= 1 && argc == 5 + 2 * count && std::string(argv[4 + 2 * count]) == "loop";
    const bool ring = loop || (count >= 1 && argc == 5 + 2 * count && std::string(argv[4 + 2 * count]) == "ring");
    if (count < 1 || argc < 2 + 2 * count || (argc > 4 + 2 * count && !ring) || (ring && count < 3)) {
        std::fprintf(stderr, "usage: %s k a1.bin .. ak.bin b1.bin .. bk.bin [cloud.ply [adjust_iterations [ring | loop]]]   (k >= 1; ring, loop: k >= 3)\n", argv[0]);
        return 2;
    }
    const char *ply = argc >= 3 + 2 * count ? argv[2 + 2 * count] : "fused_cloud.ply";
    const int adjust_iterations = argc >= 4 + 2 * count ? std::atoi(argv[3 + 2 * count]) : 0;
    const unsigned w = 720, h = 576;                        // the dino frames
    float K[9] = { 2360.0f, 0, (float)(w / 2.0), 0, 2360, (float)(h / 2.0), 0, 0, 1 };
    float inv_K[9] = { (float)(1.0 / 2360), 0, (float)(-(w / 2.0) / 2360), 0, (float)(1.0 / 2360), (float)(-(h / 2.0) / 2360), 0, 0, 1 };

    std::vector<std::vector<SiftPoint>> fa, fb;
    for (int k = 0; k < count; ++k) { fa.push_back(read_sift(argv[2 + k])); fb.push_back(read_sift(argv[2 + count + k])); }
    for (int k = 0; k + (ring ? 0 : 1) < count; ++k) {      // a link follows match indices: b_k and a_{k+1} are one view's records
        const std::vector<SiftPoint> &x = fb[(size_t)k], &y = fa[(size_t)(k + 1) % (size_t)count];
        bool same = x.size() == y.size();
        for (size_t j = 0; same && j < x.size(); ++j) same = x[j].xpos == y[j].xpos && x[j].ypos == y[j].ypos;
        if (!same) {
            std::fprintf(stderr, "%s and %s are not the records of one view (count or positions differ)\n", argv[2 + count + k], argv[2 + (k + 1) % count]);
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
    SfM::ClosedRing closed;
    if (ring) {
        static const char *const status[3] = { "closed", "open", "rejected" };
        closed = SfM::close_ring(pairs.data(), records.data(), count);
        const sfm_ring_report &rr = closed.report;
        std::printf("ring: %s, drift s %.6g rot %.6g rad, seam rms %.6g -> %.6g px (link %.6g), %d records\n", status[rr.status],
                    std::exp((double)rr.drift_log_scale), (double)rr.drift_rotation_rad, (double)rr.seam_rms_open_px, (double)rr.seam_rms_closed_px,
                    (double)rr.seam_rms_link_px, rr.seam_count);
    }
    SfM::FusedRing fused;
    if (loop) fused = SfM::fuse_ring(pairs.data(), records.data(), count, closed.corrected.data());
    const SfM::FusedModel model = loop ? fused.model : SfM::fuse_chain(pairs.data(), records.data(), count, 5, 4.0f, ring ? closed.corrected.data() : nullptr);
    std::printf("fuse: %d tracks, %d observations, %d refined, %d kept, %d segments, longest track %d views\n", model.tracks, model.observations,
                model.refined, model.kept, model.segments, model.longest_track);
    if (loop) {
        static const char *const status[3] = { "closed", "open", "rejected" };
        const sfm_fuse_ring_report &fr = fused.report;
        std::printf("seam: %s, closure s %.6g rot %.6g rad t %.6g, %d proposals, %d ineligible, %d seam tracks, %d refined, %d kept\n", status[fr.status],
                    std::exp((double)fr.closure_log_scale), (double)fr.closure_rotation_rad, (double)fr.closure_t, fr.seam_proposals, fr.seam_ineligible,
                    fr.seam_tracks, fr.seam_refined, fr.seam_kept);
    }

    const int T = model.tracks;
    std::vector<float> points = model.points;
    if (adjust_iterations > 0) {
        const SfM::AdjustedChain adj = SfM::adjust_chain(pairs.data(), count, model, adjust_iterations);
        for (int i = 0; i < count; ++i) {
            const sfm_adjust_chain_report &rep = adj.reports[(size_t)i];
            if (rep.root != i) continue;
            std::printf("chain adjust: segment %d: %d cameras, %d tracks, rms %.6g -> %.6g px, %d iterations\n", rep.root, rep.num_cameras,
                        rep.num_tracks, (double)rep.initial_rms_px, (double)rep.final_rms_px, rep.iterations);
        }
        points = adj.points;
        std::vector<float> cams = adj.cams;
        std::vector<uint8_t> used = adj.used;
        if (loop && fused.report.status == SFM_RING_CLOSED) {          // the ring's own adjustment: one camera per view, the seam tracks used
            const SfM::AdjustedRing ra = SfM::adjust_ring(pairs.data(), count, fused, adjust_iterations);
            const sfm_adjust_ring_report &rep = ra.report;
            std::printf("ring adjust: %d cameras, %d tracks, %d seam tracks, rms %.6g -> %.6g px, %d iterations\n", rep.num_cameras, rep.num_tracks,
                        rep.num_seam_tracks, (double)rep.initial_rms_px, (double)rep.final_rms_px, rep.iterations);
            points = ra.points; cams = ra.cams; used = ra.used;
        }
        // the tracks the last adjustment did not use, under its cameras: one consistent cloud
        const SfM::IntersectedTracks it = SfM::intersect_tracks(pairs.data(), count, model, cams.data(), points.data(), used.data());
        std::fprintf(stderr, "intersect: %d tracks, %d intersected, %d refined, %d kept, %d copied, %d from the linear start, %d without a start, %d promoted\n",
                    it.counts[0], it.counts[1], it.counts[2], it.counts[3], it.counts[4], it.counts[5], it.counts[6], it.counts[7]);
        points = it.points;
    }

    // the first segment's tracks: one point each
    std::vector<float> cloud;                               // x, y, z per point
    for (int t = 0; t < T; ++t) {
        const int pair = model.obs_cam[(size_t)model.track_offset[(size_t)t]] >> 1;
        if (model.root[(size_t)pair] != 0) continue;
        for (int c = 0; c < 3; ++c) cloud.push_back(points[(size_t)c * T + t]);
    }
    const int total = (int)(cloud.size() / 3);
    std::vector<float> cols((size_t)4 * total, 1.0f);       // WritePLY's 4 x N layout
    for (int j = 0; j < total; ++j)
        for (int c = 0; c < 3; ++c) cols[(size_t)c * total + j] = cloud[(size_t)3 * j + c];
    const int written = WritePLY(ply, cols.data(), total);
    std::printf("fused cloud: %d points -> %s\n", written, ply);
    owned.clear();
    for (SiftData &s : sift) FreeSiftData(s);
    return 0;
}
