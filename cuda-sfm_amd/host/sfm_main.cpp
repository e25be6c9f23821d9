// sfm_main.cpp -- the reference application's compute path, start to end (src/main.cpp:249-307), on the
// MI355X: read two grey images, ExtractSift x2, MatchSiftData, K / K^-1, SfM::Image_pair -> fillXU ->
// estimateE -> computePosecandidates -> choosePose -> linear_triangulation.  The GL viewer that follows
// in the reference (main.cpp:308-340) is replaced by a PLY file.
//     sfm_main <img1.pgm|ppm> <img2.pgm|ppm> <cloud.ply> [result.bin] [num_hypotheses] [pose_mode] [thresh] [initBlur] [focal]
//              [refine_iterations] [img3.pgm|ppm]
// refine_iterations > 0 (default 0: nothing changes): two-view bundle adjustment after the pose chain; the PLY then holds the
// refined points of the correspondences the refinement used, and one more line is printed.
// img3 (with refine_iterations > 0): a third view of the same size, registered against the refined points (image 1 matched
// against it, P3P RANSAC + pose LM); one more line: inliers / candidates, rms before -> after, |C3| = |-R3^T t3|.  Then the pair's
// points are triangulated / refined over the three views; one more line: view3 points: <new> new, <refined> refined, <kept> kept,
// <rejected> rejected; the PLY is then written again with the merged cloud (new and refined points from the three-view result, the
// rest as before) and a last line says so: merged cloud: <count> points -> <file>.  In front of that line both cameras and the
// points are adjusted over the three views (sfm_adjust_view) and the points triangulated once more with the adjusted cameras; two
// lines: adjust: <points> points (<v2> / <v3> in views 2 / 3), rms <a> -> <b> px, <k> iterations, and adjusted view3 points:
// with the four counts again.  The PLY holds the records of the first triangulation at their adjusted positions.
// result.bin (optional, for tests): int n, float E[9], int pose, uint hyp, uint count, float P[16] (chosen), float pts[4n], u8 mask[n]
// Plain C++: facade headers + libsfm_amd.so only (no OpenCV, no GL).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>

#include "cudaImage.h"
#include "sfm.h"
#include "sfm_io.h"

int main(int argc, char **argv)
{
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s img1 img2 cloud.ply [result.bin] [num_hypotheses] [pose_mode] [thresh] [initBlur] [focal] [refine_iterations] [img3]\n", argv[0]);
        return 2;
    }
    std::vector<float> limg, rimg;
    int wi = 0, hi = 0, w2 = 0, h2 = 0;
    if (!ReadPNM(argv[1], limg, wi, hi) || !ReadPNM(argv[2], rimg, w2, h2) || wi != w2 || hi != h2) {
        std::fprintf(stderr, "cannot read two equally sized P5/P6 images\n");
        return 2;
    }
    const unsigned int w = (unsigned)wi, h = (unsigned)hi;
    std::cout << "Image size = (" << w << "," << h << ")" << std::endl;
    const int devNum = 0;

    std::cout << "Initializing data..." << std::endl;                              // main.cpp:259-266
    InitCuda(devNum);
    CudaImage img1, img2;
    img1.Allocate(w, h, iAlignUp(w, 128), false, NULL, limg.data());
    img2.Allocate(w, h, iAlignUp(w, 128), false, NULL, rimg.data());
    img1.Download();
    img2.Download();

    SiftData siftData1, siftData2;                                                 // main.cpp:268-279
    float initBlur = argc > 8 ? std::strtof(argv[8], nullptr) : 1.5f;
    float thresh = argc > 7 ? std::strtof(argv[7], nullptr) : 1.0f;
    InitSiftData(siftData1, 32768, true, true);
    InitSiftData(siftData2, 32768, true, true);
    float *memoryTmp = AllocSiftTempMemory(w, h, 5, false);
    // main.cpp:273-274 calls ExtractSift twice in a row; the pair form issues both at once (same results)
    ExtractSiftPair(siftData1, siftData2, img1, img2, 5, initBlur, thresh, 0.0f, false, memoryTmp);
    FreeSiftTempMemory(memoryTmp);

    MatchSiftData(siftData1, siftData2);                                           // main.cpp:282

    const float focal = argc > 9 ? std::strtof(argv[9], nullptr) : 2360.0f;        // main.cpp:292-297
    float K[9] = { focal, 0, (float)(w / 2.0), 0, focal, (float)(h / 2.0), 0, 0, 1 };
    float inv_K[9] = { (float)(1.0 / focal), 0, (float)(-(w / 2.0) / focal), 0, (float)(1.0 / focal), (float)(-(h / 2.0) / focal), 0, 0, 1 };
    SfM::Image_pair sfm(K, inv_K, 2, siftData1.numPts);                            // main.cpp:298
    if (argc > 5 && std::atoi(argv[5]) > 0) sfm.ransacParams().num_hypotheses = (uint32_t)std::atoi(argv[5]);
    if (argc > 6) sfm.setPoseMode(std::atoi(argv[6]));
    sfm.fillXU(siftData1.d_data);                                                  // main.cpp:299-307
    sfm.estimateE();
    sfm.computePosecandidates();
    sfm.choosePose();
    sfm.linear_triangulation();

    const int32_t n = siftData1.numPts;
    const std::vector<float> pts = sfm.getPoints();
    const std::vector<uint8_t> mask = sfm.getInlierMask();
    const int refine_iterations = argc > 10 ? std::atoi(argv[10]) : 0;
    int written = 0;
    sfm_refine_report rep = {};
    std::vector<uint8_t> used;
    if (refine_iterations > 0) {
        rep = sfm.refine(refine_iterations);
        const std::vector<float> refined = sfm.getRefinedPoints();
        sfm.getReprojectionErrors(&used);
        written = WritePLY(argv[3], refined.data(), n, used.data());
    } else {
        written = WritePLY(argv[3], pts.data(), n, mask.data());
    }
    uint32_t hyp = 0, cnt = 0;
    sfm.getBestHypothesis(&hyp, &cnt);
    std::printf("sfm_main: %d / %d features, %u inliers of %d matches, pose %d, %d points -> %s\n", siftData1.numPts, siftData2.numPts, cnt, n,
                sfm.getPoseIndex(), written, argv[3]);
    if (refine_iterations > 0)
        std::printf("refine: %d points, rms %.4f -> %.4f px, %d iterations\n", rep.num_used, rep.initial_rms_px, rep.final_rms_px, rep.iterations);
    if (refine_iterations > 0 && argc > 11 && argv[11][0]) {
        std::vector<float> img;
        int w3 = 0, h3 = 0;
        if (!ReadPNM(argv[11], img, w3, h3) || w3 != wi || h3 != hi) {
            std::fprintf(stderr, "cannot read %s as an image of the size of the other two\n", argv[11]);
            return 2;
        }
        CudaImage img3;
        img3.Allocate(w, h, iAlignUp(w, 128), false, NULL, img.data());
        img3.Download();
        SiftData siftData3;
        InitSiftData(siftData3, 32768, true, true);
        float *tmp = AllocSiftTempMemory(w, h, 5, false);
        ExtractSift(siftData3, img3, 5, initBlur, thresh, 0.0f, false, tmp);
        FreeSiftTempMemory(tmp);
        MatchSiftData(siftData1, siftData3);                                        // rewrites image 1's match fields only
        const sfm_register_report vr = sfm.registerView(siftData1.d_data);
        float P3[16];
        sfm.getViewPose(P3);
        double c3[3], nc = 0.0;
        for (int a = 0; a < 3; ++a) {
            c3[a] = -((double)P3[a] * P3[3] + (double)P3[4 + a] * P3[7] + (double)P3[8 + a] * P3[11]);
            nc += c3[a] * c3[a];
        }
        std::printf("view3: %d/%d inliers, rms %.4f -> %.4f px, |C3| %.4f\n", vr.num_inliers, vr.num_candidates, vr.initial_rms_px,
                    vr.final_rms_px, std::sqrt(nc));
        // the intersection step behind the resection: the merged cloud replaces the two-view one in the PLY -- new and refined
        // points from the three-view result, the rest as before
        const SfM::ViewPoints cloud = sfm.triangulateView(siftData1.d_data);
        std::printf("view3 points: %d new, %d refined, %d kept, %d rejected\n", cloud.counts[SFM_VP_NEW], cloud.counts[SFM_VP_REFINED],
                    cloud.counts[SFM_VP_KEPT], cloud.counts[SFM_VP_NEW_REJECTED]);
        const SfM::ViewAdjust adj = sfm.adjustView(siftData1.d_data, cloud);
        std::printf("adjust: %d points (%d / %d in views 2 / 3), rms %.4f -> %.4f px, %d iterations\n", adj.report.num_points, adj.report.num_view2,
                    adj.report.num_view3, adj.report.initial_rms_px, adj.report.final_rms_px, adj.report.iterations);
        const SfM::ViewPoints again = sfm.triangulateView(siftData1.d_data, 5, 4.0f, 1.0f, adj.poses);
        std::printf("adjusted view3 points: %d new, %d refined, %d kept, %d rejected\n", again.counts[SFM_VP_NEW], again.counts[SFM_VP_REFINED],
                    again.counts[SFM_VP_KEPT], again.counts[SFM_VP_NEW_REJECTED]);
        std::vector<uint8_t> keep(used);
        for (int32_t j = 0; j < n; ++j)
            if (cloud.flags[(size_t)j] == SFM_VP_NEW || cloud.flags[(size_t)j] == SFM_VP_REFINED) keep[(size_t)j] = 1;
        // the records are those of the first triangulation; their positions are the adjusted ones (a record the adjustment did not
        // use keeps the triangulation's column, and so does every record when the adjustment is degenerate)
        const int merged = WritePLY(argv[3], adj.points.data(), n, keep.data());        // replaces the two-view file written above
        std::printf("merged cloud: %d points -> %s\n", merged, argv[3]);
        FreeSiftData(siftData3);
    }
    if (argc > 4 && argv[4][0]) {
        float E[9], P[64];
        sfm.getE(E); sfm.getPoseCandidates(P);
        const int32_t pind = sfm.getPoseIndex();
        FILE *o = std::fopen(argv[4], "wb");
        if (!o) { std::perror(argv[4]); return 2; }
        std::fwrite(&n, 4, 1, o); std::fwrite(E, 4, 9, o); std::fwrite(&pind, 4, 1, o); std::fwrite(&hyp, 4, 1, o); std::fwrite(&cnt, 4, 1, o);
        std::fwrite(P + 16 * (pind >= 0 && pind < 4 ? pind : 0), 4, 16, o);
        std::fwrite(pts.data(), 4, pts.size(), o); std::fwrite(mask.data(), 1, mask.size(), o);
        std::fclose(o);
    }
    FreeSiftData(siftData1);
    FreeSiftData(siftData2);
    return 0;
}
