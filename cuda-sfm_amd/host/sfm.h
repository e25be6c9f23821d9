// sfm.h -- host-side mirror of the reference's SfM::Image_pair (SfM/sfm.h:20-60, SfM/sfm.cu:28-359):
// same class name, constructor signature, method names and call order as the reference's caller uses
// them (src/main.cpp:298-307), implemented on the C ABI of include/sfm_amd.h.
//
//     SfM::Image_pair sfm(K, inv_K, 2, siftData1.numPts);
//     sfm.fillXU(siftData1.d_data);
//     sfm.estimateE();
//     sfm.computePosecandidates();
//     sfm.choosePose();
//     sfm.linear_triangulation();
//
// Additions (the reference keeps its results private and only leaks them through a GL VBO copy,
// sfm.cu:374-383): get* accessors, setRansacParams, setPoseMode and both spellings of the two
// BASELINE names (computePoseCandidates / linearTriangulate).
#ifndef SFM_AMD_SFM_H
#define SFM_AMD_SFM_H

#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "cudaSift.h"

namespace SfM {

// what triangulateView / triangulate_views return for one pair, in host memory
struct ViewPoints {
    std::vector<float> points;          // 4 x N: (X, Y, Z, 1) where flags is SFM_VP_NEW / SFM_VP_REFINED, else the refined point
    std::vector<uint8_t> flags;         // N: SFM_VP_*
    int32_t counts[8];                  // [0..4]: points per class
};

// what adjustView / adjust_views return for one pair, in host memory
struct ViewAdjust {
    float poses[24];                    // adjusted [R|t] of cameras 2 and 3: R (9, row-major) then t (3), each
    std::vector<float> points;          // 4 x N: (X, Y, Z, 1) for used records, the input column otherwise
    std::vector<uint8_t> views;         // N: bit 0 / 1 / 2 = views 1 / 2 / 3 used, 0 = record not used
    sfm_adjust_report report;
};

// A similarity X' = s R X + t (R row-major), host arithmetic in double: the link between two pairs' frames and its compositions.
struct Sim3 {
    double s = 1.0;
    double R[9] = { 1, 0, 0, 0, 1, 0, 0, 0, 1 };
    double t[3] = { 0, 0, 0 };
    static Sim3 from(const float sim[13])              // s, R (9), t (3) as sfm_align_out.d_sim holds them
    {
        Sim3 r;
        r.s = sim[0];
        for (int k = 0; k < 9; ++k) r.R[k] = sim[1 + k];
        for (int k = 0; k < 3; ++k) r.t[k] = sim[10 + k];
        return r;
    }
    void apply(const double X[3], double Y[3]) const
    {
        for (int r = 0; r < 3; ++r) Y[r] = s * (R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2]) + t[r];
    }
    // this after first: X -> s R (s1 R1 X + t1) + t
    Sim3 compose(const Sim3 &first) const
    {
        Sim3 r;
        r.s = s * first.s;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) r.R[3 * i + j] = R[3 * i] * first.R[j] + R[3 * i + 1] * first.R[3 + j] + R[3 * i + 2] * first.R[6 + j];
        apply(first.t, r.t);
        return r;
    }
    Sim3 inverse() const                               // X = (1 / s) R^T (X' - t)
    {
        Sim3 r;
        r.s = 1.0 / s;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) r.R[3 * i + j] = R[3 * j + i];
        for (int i = 0; i < 3; ++i) r.t[i] = -r.s * (r.R[3 * i] * t[0] + r.R[3 * i + 1] * t[1] + r.R[3 * i + 2] * t[2]);
        return r;
    }
};

// what alignTo / align_pairs return for one link, in host memory
struct PairLink {
    Sim3 sim, ransac;                   // X_other = s R X_this + t: refined, and the RANSAC winner's
    std::vector<uint8_t> inlier;        // N of this pair: the final mask
    sfm_align_report report;
};

namespace detail {
// a device allocation that is freed when it goes out of scope, also when a facade call throws (SFM_FACADE_THROW)
struct DeviceBlock {
    char *p = nullptr;
    explicit DeviceBlock(size_t bytes) { SFM_FACADE_CALL(sfm_device_alloc(sfm_facade::context(), bytes, reinterpret_cast<void **>(&p))); }
    DeviceBlock(const DeviceBlock &) = delete;
    DeviceBlock &operator=(const DeviceBlock &) = delete;
    ~DeviceBlock() { if (p) sfm_device_free(sfm_facade::context(), p); }
};

// device scratch of one triangulation result: points, flags and counts in ONE sfm_device_alloc block
struct ViewPointsScratch {
    char *block = nullptr;
    size_t n = 0;
    explicit ViewPointsScratch(int num_points) : n((size_t)num_points)
    {
        SFM_FACADE_CALL(sfm_device_alloc(sfm_facade::context(), 16 * n + 32 + flag_bytes(), reinterpret_cast<void **>(&block)));
    }
    ViewPointsScratch(const ViewPointsScratch &) = delete;
    ViewPointsScratch &operator=(const ViewPointsScratch &) = delete;
    ~ViewPointsScratch() { if (block) sfm_device_free(sfm_facade::context(), block); }
    size_t flag_bytes() const { return (n + 15) / 16 * 16; }
    sfm_view_points_out out() const
    {
        sfm_view_points_out o;
        o.d_points = reinterpret_cast<float *>(block);
        o.d_counts = reinterpret_cast<int32_t *>(block + 16 * n);
        o.d_flags = reinterpret_cast<uint8_t *>(block + 16 * n + 32);
        o.d_err = nullptr;
        return o;
    }
    ViewPoints download() const          // synchronises
    {
        ViewPoints r;
        r.points.resize(4 * n); r.flags.resize(n);
        const sfm_view_points_out o = out();
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.points.data(), o.d_points, 16 * n));
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.flags.data(), o.d_flags, n));
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.counts, o.d_counts, 32));
        return r;
    }
};
// device scratch of one adjustment: the triangulation's points and flags uploaded, the outputs, in ONE sfm_device_alloc block
struct AdjustScratch {
    size_t n = 0;
    DeviceBlock mem;
    char *block = nullptr;
    // vp must be the triangulation of this pair: 4 x num_points points and num_points flags (SFM_E_INVALID otherwise)
    AdjustScratch(int num_points, const ViewPoints &vp) : n((size_t)num_points), mem(32 * n + 96 + 48 + 2 * flag_bytes()), block(mem.p)
    {
        if (vp.points.size() != 4 * n || vp.flags.size() != n)
            sfm_facade::fail("adjustView: the ViewPoints do not have the pair's number of points", SFM_E_INVALID);
        if (n) {
            SFM_FACADE_CALL(sfm_copy_to_device(sfm_facade::context(), block, vp.points.data(), 16 * n));
            SFM_FACADE_CALL(sfm_copy_to_device(sfm_facade::context(), block + 32 * n + 144, vp.flags.data(), n));
        }
    }
    size_t flag_bytes() const { return (n + 16) / 16 * 16; }      // never 0: the flags and the view bits get addresses of their own
    sfm_adjust_in in(const SiftPoint *data) const
    {
        sfm_adjust_in i;
        i.d_sift = reinterpret_cast<const sfm_sift_point *>(data);
        i.d_points = reinterpret_cast<const float *>(block);
        i.d_flags = reinterpret_cast<const uint8_t *>(block + 32 * n + 144);
        return i;
    }
    sfm_adjust_out out() const
    {
        sfm_adjust_out o;
        o.d_points = reinterpret_cast<float *>(block + 16 * n);
        o.d_poses = reinterpret_cast<float *>(block + 32 * n);
        o.d_report = reinterpret_cast<sfm_adjust_report *>(block + 32 * n + 96);
        o.d_views = reinterpret_cast<uint8_t *>(block + 32 * n + 144 + flag_bytes());
        o.d_err = nullptr;
        return o;
    }
    ViewAdjust download() const          // synchronises
    {
        ViewAdjust r;
        r.points.resize(4 * n); r.views.resize(n);
        const sfm_adjust_out o = out();
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.points.data(), o.d_points, 16 * n));
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.views.data(), o.d_views, n));
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.poses, o.d_poses, sizeof(r.poses)));
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), &r.report, o.d_report, sizeof(r.report)));
        return r;
    }
};
// device scratch of one link: the index built from the records, the outputs, in ONE sfm_device_alloc block
struct AlignScratch {
    size_t n = 0;
    DeviceBlock mem;
    explicit AlignScratch(int num_points) : n((size_t)num_points), mem(4 * n + 112 + 48 + n + 16) {}
    int32_t *index() const { return reinterpret_cast<int32_t *>(mem.p + 160); }
    sfm_align_out out() const
    {
        sfm_align_out o;
        o.d_sim = reinterpret_cast<float *>(mem.p);
        o.d_report = reinterpret_cast<sfm_align_report *>(mem.p + 112);
        o.d_inlier = reinterpret_cast<uint8_t *>(mem.p + 160 + 4 * n);
        o.d_err = nullptr;
        o.d_counts = nullptr;
        return o;
    }
    PairLink download() const            // synchronises
    {
        PairLink r;
        float sim[26];
        r.inlier.resize(n);
        const sfm_align_out o = out();
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), sim, o.d_sim, sizeof(sim)));
        if (n) SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), r.inlier.data(), o.d_inlier, n));
        SFM_FACADE_CALL(sfm_copy_to_host(sfm_facade::context(), &r.report, o.d_report, sizeof(r.report)));
        r.sim = Sim3::from(sim);
        r.ransac = Sim3::from(sim + 13);
        return r;
    }
};
} // namespace detail

class Image_pair {
    sfm_pair *pair_ = nullptr;
    float *d_F_ = nullptr;                     // fundamental()'s result, allocated at its first call
    int num_points_ = 0;
    int pose_mode_ = SFM_POSE_REFERENCE;       // drop-in default: the reference's own behaviour
    sfm_ransac_params params_;
public:
    Image_pair(float k[9], float k_inv[9], int image_count, int num_points) : num_points_(num_points)
    {
        SFM_FACADE_CALL(sfm_pair_create(sfm_facade::context(), k, k_inv, image_count, num_points, &pair_));
        sfm_ransac_default_params(&params_, num_points);      // H = N/8, thr 1e-6 (sfm.cu:95,220)
    }
    Image_pair(const Image_pair &) = delete;
    Image_pair &operator=(const Image_pair &) = delete;
    ~Image_pair() { if (d_F_) sfm_device_free(sfm_facade::context(), d_F_); if (pair_) sfm_pair_destroy(pair_); }

    // ---- the reference's call surface --------------------------------------------------------
    void fillXU(SiftPoint *data) { SFM_FACADE_CALL(sfm_fill_xu(pair_, data)); }               // sfm.cu:80-92
    void estimateE() { SFM_FACADE_CALL(sfm_estimate_E(pair_, &params_)); }                    // sfm.cu:94-153
    void computePosecandidates() { SFM_FACADE_CALL(sfm_pose_candidates(pair_, pose_mode_)); } // sfm.cu:238-252
    void choosePose() { SFM_FACADE_CALL(sfm_choose_pose(pair_, pose_mode_)); }                // sfm.cu:254-307
    void linear_triangulation() { SFM_FACADE_CALL(sfm_triangulate(pair_, pose_mode_)); }      // sfm.cu:309-344
#ifdef SFM_AMD_COMM_H
    // multi-GPU estimateE (include sfm_amd_comm.h first): num_hypotheses is the global count, every rank calls it
    void estimateE(sfm_comm *comm) { SFM_FACADE_CALL(sfm_estimate_E_sharded(pair_, &params_, comm)); }
#endif
    void computePoseCandidates() { computePosecandidates(); }
    void linearTriangulate() { linear_triangulation(); }

    // ---- additions ----------------------------------------------------------------------------
    sfm_ransac_params &ransacParams() { return params_; }
    void setRansacParams(uint32_t num_hypotheses, float threshold, uint32_t seed, const int32_t *d_indices = nullptr)
    {
        params_.num_hypotheses = num_hypotheses; params_.threshold = threshold; params_.seed = seed; params_.d_indices = d_indices;
        params_.hyp_begin = 0; params_.hyp_count = 0;
    }
    void setPoseMode(int mode) { pose_mode_ = mode; }
    // computePosecandidates + choosePose + linear_triangulation (src/main.cpp:302-306) as one launch; same results
    void poseChain() { SFM_FACADE_CALL(sfm_pose_chain(pair_, pose_mode_)); }
    // another correspondence set of at most the constructor's num_points, without re-allocating anything
    void reset(int num_points)
    {
        SFM_FACADE_CALL(sfm_pair_reset(pair_, num_points));
        num_points_ = num_points;
        sfm_ransac_default_params(&params_, num_points);
    }
    void getResult(float record[28]) { SFM_FACADE_CALL(sfm_get_result(pair_, record)); }
    int numPoints() const { return num_points_; }
    sfm_pair *handle() { return pair_; }

    void getE(float E[9]) { SFM_FACADE_CALL(sfm_get_E(pair_, E)); }
    void getBestHypothesis(uint32_t *hyp, uint32_t *count) { SFM_FACADE_CALL(sfm_get_best(pair_, hyp, count)); }
    std::vector<int32_t> getInlierCounts()
    {
        std::vector<int32_t> c(params_.hyp_count ? params_.hyp_count : params_.num_hypotheses - params_.hyp_begin);
        SFM_FACADE_CALL(sfm_get_inlier_counts(pair_, c.data(), c.size()));
        return c;
    }
    std::vector<uint8_t> getInlierMask()
    {
        std::vector<uint8_t> m((size_t)num_points_);
        SFM_FACADE_CALL(sfm_get_inlier_mask(pair_, m.data()));
        return m;
    }
    void getPoseCandidates(float P[64]) { SFM_FACADE_CALL(sfm_get_pose_candidates(pair_, P)); }
    void getPoseInverses(float P[64]) { SFM_FACADE_CALL(sfm_get_pose_inverses(pair_, P)); }
    int getPoseIndex() { int i = 0; SFM_FACADE_CALL(sfm_get_pose_index(pair_, &i)); return i; }
    // sfm.cu:374-383: (x, y, z, 1) vertices and the constant colour buffer, into DEVICE buffers of 4 * N floats
    void copyBoidsToVBO(float *vbodptr_positions, float *vbodptr_velocities)
    {
        SFM_FACADE_CALL(sfm_copy_points_to_vbo(pair_, vbodptr_positions, vbodptr_velocities, 1.0f));
        SFM_FACADE_CALL(sfm_ctx_synchronize(sfm_facade::context()));            // cudaDeviceSynchronize of sfm.cu:382
    }
    std::vector<float> getPoints()          // 4 x N row-major [x; y; z; 1] (d_final_points, sfm.cu:77,335)
    {
        std::vector<float> p((size_t)4 * num_points_);
        SFM_FACADE_CALL(sfm_get_points(pair_, p.data()));
        return p;
    }
    // two-view bundle adjustment after estimateE (sfm_refine_two_view): camera 2's pose and the inliers' points by
    // Levenberg-Marquardt on Huber-weighted pixel residuals; returns the report (synchronises)
    sfm_refine_report refine(int max_iterations = 20, float huber_px = 1.0f)
    {
        sfm_refine_params p;
        sfm_refine_default_params(&p);
        p.max_iterations = max_iterations;
        p.huber_px = huber_px;
        SFM_FACADE_CALL(sfm_refine_two_view(pair_, &p));
        return getRefineReport();
    }
    sfm_refine_report getRefineReport() { sfm_refine_report r; SFM_FACADE_CALL(sfm_get_refine_report(pair_, &r)); return r; }
    void getRefinedPose(float P[16], float E[9]) { SFM_FACADE_CALL(sfm_get_refined_pose(pair_, P, E)); }   // [R|t; 0 0 0 1], [t]x R
    // the pair's fundamental matrix for MatchSiftDataGuided (sfm_pair_fundamental): 9 DEVICE floats owned by the pair, from the
    // refined E or (refined = false) the E of estimateE; view 1 = the records' (xpos, ypos).  Enqueue only; each call overwrites it.
    const float *fundamental(bool refined = true)
    {
        if (!d_F_) SFM_FACADE_CALL(sfm_device_alloc(sfm_facade::context(), 9 * sizeof(float), (void **)&d_F_));
        SFM_FACADE_CALL(sfm_pair_fundamental(pair_, refined ? 1 : 0, d_F_));
        return d_F_;
    }
    std::vector<float> getRefinedPoints()   // 4 x N: used points refined, the others triangulated against the refined pose
    {
        std::vector<float> p((size_t)4 * num_points_);
        SFM_FACADE_CALL(sfm_get_refined_points(pair_, p.data()));
        return p;
    }
    std::vector<float> getReprojectionErrors(std::vector<uint8_t> *used = nullptr)     // px per point; used flags on request
    {
        std::vector<float> e((size_t)num_points_);
        if (used) used->resize((size_t)num_points_);
        SFM_FACADE_CALL(sfm_get_reprojection_errors(pair_, e.data(), used ? used->data() : nullptr));
        return e;
    }
    // registers a further view against the refined points (sfm_register_view): data = image 1's records re-matched against
    // it (MatchSiftData(image 1, view)); P3P RANSAC, then the pose LM; returns the report (synchronises)
    sfm_register_report registerView(SiftPoint *data, int max_iterations = 10, float threshold_px = 4.0f)
    {
        sfm_register_params p;
        sfm_register_default_params(&p);
        p.max_iterations = max_iterations;
        p.threshold_px = threshold_px;
        SFM_FACADE_CALL(sfm_register_view(pair_, reinterpret_cast<const sfm_sift_point *>(data), &p));
        sfm_register_report r;
        SFM_FACADE_CALL(sfm_get_register_report(pair_, &r));
        return r;
    }
    void getViewPose(float P[16], float P_ransac[16] = nullptr) { SFM_FACADE_CALL(sfm_get_view_pose(pair_, P, P_ransac)); }   // [R3|t3; 0 0 0 1]
    std::vector<float> getViewErrors(std::vector<uint8_t> *inlier = nullptr)     // px per point (+inf: no candidate); mask on request
    {
        std::vector<float> e((size_t)num_points_);
        if (inlier) inlier->resize((size_t)num_points_);
        SFM_FACADE_CALL(sfm_get_view_errors(pair_, e.data(), inlier ? inlier->data() : nullptr));
        return e;
    }
    // the pair's points triangulated / refined over views 1, 2 and the registered view (sfm_triangulate_view): data = the
    // records registerView took; nothing in the pair changes; returns points, flags and counts (synchronises)
    // poses: null, or 24 floats in HOST memory -- [R|t] of cameras 2 and 3 as ViewAdjust::poses holds them -- instead of the
    // refined pose and the registered view's
    ViewPoints triangulateView(SiftPoint *data, int max_iterations = 5, float threshold_px = 4.0f, float min_parallax_deg = 1.0f,
                               const float *poses = nullptr)
    {
        sfm_view_points_params p;
        sfm_view_points_default_params(&p);
        p.max_iterations = max_iterations;
        p.threshold_px = threshold_px;
        p.min_parallax_deg = min_parallax_deg;
        const detail::ViewPointsScratch scratch(num_points_);
        const sfm_view_points_out out = scratch.out();
        std::unique_ptr<detail::DeviceBlock> d_poses;
        if (poses) {
            d_poses.reset(new detail::DeviceBlock(24 * sizeof(float)));
            SFM_FACADE_CALL(sfm_copy_to_device(sfm_facade::context(), d_poses->p, poses, 24 * sizeof(float)));
            p.d_poses = reinterpret_cast<const float *>(d_poses->p);
        }
        SFM_FACADE_CALL(sfm_triangulate_view(pair_, reinterpret_cast<const sfm_sift_point *>(data), &p, &out));
        return scratch.download();
    }
    // both cameras and every used point adjusted over views 1, 2 and the registered view (sfm_adjust_view): data = the records
    // registerView took, vp = what triangulateView returned for them; nothing in the pair changes; returns the adjusted poses,
    // points, view bits and the report (synchronises)
    ViewAdjust adjustView(SiftPoint *data, const ViewPoints &vp, int max_iterations = 20, float huber_px = 1.0f)
    {
        sfm_adjust_params p;
        sfm_adjust_default_params(&p);
        p.max_iterations = max_iterations;
        p.huber_px = huber_px;
        const detail::AdjustScratch scratch(num_points_, vp);
        const sfm_adjust_in in = scratch.in(data);
        const sfm_adjust_out out = scratch.out();
        SFM_FACADE_CALL(sfm_adjust_view(pair_, &in, &p, &out));
        return scratch.download();
    }
    // the similarity that carries this pair's frame into `other`'s (sfm_align_pair): data = the records fillXU took (image 1
    // matched against image 2, which is image 1 of `other`); both pairs refined; nothing in either pair changes; returns the
    // link, the final mask and the report (synchronises)
    PairLink alignTo(Image_pair &other, SiftPoint *data, int max_iterations = 10, float threshold_px = 4.0f)
    {
        sfm_align_params p;
        sfm_align_default_params(&p);
        p.max_iterations = max_iterations;
        p.threshold_px = threshold_px;
        const detail::AlignScratch scratch(num_points_);
        const sfm_align_out out = scratch.out();
        SFM_FACADE_CALL(sfm_align_index_from_matches(sfm_facade::context(), reinterpret_cast<const sfm_sift_point *>(data), num_points_, 0.85f, 0.95f,
                                                     scratch.index()));
        SFM_FACADE_CALL(sfm_align_pair(pair_, other.pair_, scratch.index(), &p, &out));
        return scratch.download();
    }
    std::vector<float> getX(int image)      // 3 x N normalised coordinates of image 0 / 1
    {
        std::vector<float> x((size_t)3 * num_points_);
        SFM_FACADE_CALL(sfm_get_XU(pair_, image == 0 ? SFM_BUF_X0 : SFM_BUF_X1, x.data()));
        return x;
    }
};

// two-view bundle adjustment of many pairs in one batched call (sfm_refine_pairs): every pair is left as its own refine() leaves
// it, bit for bit; returns the reports in the order of the list (one wait for the device)
inline std::vector<sfm_refine_report> refine_pairs(Image_pair *const *pairs, int count, int max_iterations = 20, float huber_px = 1.0f)
{
    sfm_refine_params p;
    sfm_refine_default_params(&p);
    p.max_iterations = max_iterations;
    p.huber_px = huber_px;
    std::vector<sfm_pair *> handles;
    for (int i = 0; i < count; ++i) handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
    SFM_FACADE_CALL(sfm_refine_pairs(handles.data(), count, &p, nullptr));
    std::vector<sfm_refine_report> reports;
    for (int i = 0; i < count; ++i) reports.push_back(pairs[i]->getRefineReport());
    return reports;
}

// the fundamental matrices of many pairs in one launch (sfm_pair_fundamentals), for MatchSiftDataGuided pair by pair: 9 * count
// DEVICE floats, pair i's F at get() + 9 i, each bit-equal to that pair's own fundamental(refined); freed with the last copy of the handle
inline std::shared_ptr<float> fundamentals(Image_pair *const *pairs, int count, bool refined = true)
{
    float *d_F = nullptr;
    SFM_FACADE_CALL(sfm_device_alloc(sfm_facade::context(), (size_t)9 * sizeof(float) * (size_t)(count > 0 ? count : 1), (void **)&d_F));
    std::shared_ptr<float> owner(d_F, [](float *p) { if (p) sfm_device_free(sfm_facade::context(), p); });
    std::vector<sfm_pair *> handles;
    for (int i = 0; i < count; ++i) handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
    SFM_FACADE_CALL(sfm_pair_fundamentals(handles.data(), count, refined ? 1 : 0, d_F));
    return owner;
}

// a further view registered to each of many pairs in one batched call (sfm_register_views), on the refined points like
// registerView: data[i] = image 1's records of pair i re-matched against that pair's new view; every pair is left as its own
// registerView() leaves it, bit for bit; returns the reports in the order of the list (one wait for the device)
inline std::vector<sfm_register_report> register_views(Image_pair *const *pairs, SiftPoint *const *data, int count, int max_iterations = 10,
                                                       float threshold_px = 4.0f)
{
    sfm_register_params p;
    sfm_register_default_params(&p);
    p.max_iterations = max_iterations;
    p.threshold_px = threshold_px;
    std::vector<sfm_pair *> handles;
    std::vector<const sfm_sift_point *> records;
    for (int i = 0; i < count; ++i) {
        handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
        records.push_back(reinterpret_cast<const sfm_sift_point *>(data[i]));
    }
    SFM_FACADE_CALL(sfm_register_views(handles.data(), count, records.data(), &p, nullptr, nullptr));
    std::vector<sfm_register_report> reports;
    for (int i = 0; i < count; ++i) {
        sfm_register_report r;
        SFM_FACADE_CALL(sfm_get_register_report(handles[(size_t)i], &r));
        reports.push_back(r);
    }
    return reports;
}

// triangulateView for each of many pairs in one batched call (sfm_triangulate_views): data[i] = the records register_views took
// for pair i; returns one result per pair in the order of the list, each as its own triangulateView() gives it
inline std::vector<ViewPoints> triangulate_views(Image_pair *const *pairs, SiftPoint *const *data, int count, int max_iterations = 5,
                                                 float threshold_px = 4.0f, float min_parallax_deg = 1.0f)
{
    sfm_view_points_params p;
    sfm_view_points_default_params(&p);
    p.max_iterations = max_iterations;
    p.threshold_px = threshold_px;
    p.min_parallax_deg = min_parallax_deg;
    std::vector<sfm_pair *> handles;
    std::vector<const sfm_sift_point *> records;
    std::vector<std::unique_ptr<detail::ViewPointsScratch>> scratch;
    std::vector<sfm_view_points_out> outs;
    for (int i = 0; i < count; ++i) {
        handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
        records.push_back(reinterpret_cast<const sfm_sift_point *>(data[i]));
        scratch.emplace_back(new detail::ViewPointsScratch(pairs[i] ? pairs[i]->numPoints() : 0));
        outs.push_back(scratch.back()->out());
    }
    SFM_FACADE_CALL(sfm_triangulate_views(handles.data(), count, records.data(), &p, outs.data()));
    std::vector<ViewPoints> results;
    for (int i = 0; i < count; ++i) results.push_back(scratch[(size_t)i]->download());
    return results;
}

// adjustView for each of many pairs in one batched call (sfm_adjust_views): data[i] and vps[i] as adjustView takes them; returns
// one result per pair in the order of the list, each as its own adjustView() gives it
inline std::vector<ViewAdjust> adjust_views(Image_pair *const *pairs, SiftPoint *const *data, const ViewPoints *vps, int count,
                                            int max_iterations = 20, float huber_px = 1.0f)
{
    sfm_adjust_params p;
    sfm_adjust_default_params(&p);
    p.max_iterations = max_iterations;
    p.huber_px = huber_px;
    std::vector<sfm_pair *> handles;
    std::vector<std::unique_ptr<detail::AdjustScratch>> scratch;
    std::vector<sfm_adjust_in> ins;
    std::vector<sfm_adjust_out> outs;
    for (int i = 0; i < count; ++i) {
        handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
        scratch.emplace_back(new detail::AdjustScratch(pairs[i] ? pairs[i]->numPoints() : 0, vps[i]));
        ins.push_back(scratch.back()->in(data[i]));
        outs.push_back(scratch.back()->out());
    }
    SFM_FACADE_CALL(sfm_adjust_views(handles.data(), count, ins.data(), &p, outs.data()));
    std::vector<ViewAdjust> results;
    for (int i = 0; i < count; ++i) results.push_back(scratch[(size_t)i]->download());
    return results;
}

// alignTo for each of many links in one batched call (sfm_align_pairs): link i carries as[i]'s frame into bs[i]'s, data[i] = the
// records as[i]'s fillXU took; no pair twice in as (a pair may be b of one link and a of the next: the ring); returns one result
// per link in the order of the list, each as its own alignTo() gives it
inline std::vector<PairLink> align_pairs(Image_pair *const *as, Image_pair *const *bs, SiftPoint *const *data, int count, int max_iterations = 10,
                                         float threshold_px = 4.0f)
{
    sfm_align_params p;
    sfm_align_default_params(&p);
    p.max_iterations = max_iterations;
    p.threshold_px = threshold_px;
    std::vector<sfm_pair *> ha, hb;
    std::vector<std::unique_ptr<detail::AlignScratch>> scratch;
    std::vector<const int32_t *> indices;
    std::vector<sfm_align_out> outs;
    for (int i = 0; i < count; ++i) {
        ha.push_back(as[i] ? as[i]->handle() : nullptr);
        hb.push_back(bs[i] ? bs[i]->handle() : nullptr);
        const int n = as[i] ? as[i]->numPoints() : 0;
        scratch.emplace_back(new detail::AlignScratch(n));
        SFM_FACADE_CALL(sfm_align_index_from_matches(sfm_facade::context(), reinterpret_cast<const sfm_sift_point *>(data[i]), n, 0.85f, 0.95f,
                                                     scratch.back()->index()));
        indices.push_back(scratch.back()->index());
        outs.push_back(scratch.back()->out());
    }
    SFM_FACADE_CALL(sfm_align_pairs(ha.data(), hb.data(), count, indices.data(), &p, outs.data()));
    std::vector<PairLink> results;
    for (int i = 0; i < count; ++i) results.push_back(scratch[(size_t)i]->download());
    return results;
}

// what fuse_chain returns, in host memory: the chain of pairs (pair i = views i, i + 1) as one model per segment
struct FusedModel {
    std::vector<PairLink> links;        // count - 1: the links the chain was fused over, as align_pairs gives them
    std::vector<Sim3> frames;           // count: pair i's frame into its segment's root frame
    std::vector<int32_t> root;          // count: the first pair of pair i's segment
    std::vector<float> cams;            // 24 x count: [R|t] of pair i's camera 1, then camera 2, in the root frame
    std::vector<int32_t> track;         // N = sum of the pairs' records: the track of node (pair, record), -1 = none
    std::vector<int32_t> track_offset;  // T + 1: CSR offsets into obs_cam / obs_record
    std::vector<int32_t> obs_cam;       // M: 2 * pair + (0 | 1)
    std::vector<int32_t> obs_record;    // M: the record of that pair
    std::vector<float> points;          // 4 x T (leading dimension T): one point per track in its segment's root frame
    std::vector<uint8_t> flags;         // T: SFM_FUSE_REFINED / SFM_FUSE_KEPT (fuse_ring: also SFM_FUSE_SEAM_*)
    std::vector<float> err;             // T: largest pixel error over the track's views
    int tracks = 0, observations = 0, refined = 0, kept = 0, segments = 0, longest_track = 0;
};

namespace detail {
// fuse_chain (report == null: count - 1 links) and fuse_ring (report given: count links, link count - 1 onto pair 0) in one body;
// corrected_links: null, or 13 floats per link
inline FusedModel fuse_links(Image_pair *const *pairs, SiftPoint *const *data, int count, int max_iterations, float threshold_px,
                             const float *corrected_links, sfm_fuse_ring_report *report)
{
    FusedModel r;
    if (count <= 0) return r;
    sfm_ctx *ctx = sfm_facade::context();
    sfm_align_params ap;
    sfm_align_default_params(&ap);
    sfm_fuse_params fp;
    sfm_fuse_default_params(&fp);
    fp.max_iterations = max_iterations;
    fp.threshold_px = threshold_px;
    const int nl = report ? count : count - 1;
    size_t N = 0;
    for (int i = 0; i < count; ++i) N += pairs[i] ? (size_t)pairs[i]->numPoints() : 0;
    std::vector<sfm_pair *> ha, hb;
    std::vector<std::unique_ptr<detail::AlignScratch>> scratch;
    std::vector<std::unique_ptr<detail::DeviceBlock>> errs;
    std::vector<const int32_t *> indices;
    std::vector<sfm_align_out> aouts;
    for (int i = 0; i < nl; ++i) {
        Image_pair *b = pairs[(i + 1) % count];
        ha.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
        hb.push_back(b ? b->handle() : nullptr);
        const int n = pairs[i] ? pairs[i]->numPoints() : 0;
        scratch.emplace_back(new detail::AlignScratch(n));
        errs.emplace_back(new detail::DeviceBlock(4 * (size_t)n + 16));
        SFM_FACADE_CALL(sfm_align_index_from_matches(ctx, reinterpret_cast<const sfm_sift_point *>(data[i]), n, 0.85f, 0.95f, scratch.back()->index()));
        indices.push_back(scratch.back()->index());
        sfm_align_out o = scratch.back()->out();
        o.d_err = reinterpret_cast<float *>(errs.back()->p);
        aouts.push_back(o);
    }
    if (nl > 0) SFM_FACADE_CALL(sfm_align_pairs(ha.data(), hb.data(), nl, indices.data(), &ap, aouts.data()));
    std::unique_ptr<detail::DeviceBlock> given;            // the corrected links: ONE upload, read in place of the aligned ones
    if (corrected_links && nl > 0) {
        given.reset(new detail::DeviceBlock(52 * (size_t)nl));
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, given->p, corrected_links, 52 * (size_t)nl));
    }
    std::vector<sfm_fuse_pair_in> pin((size_t)count);
    std::vector<sfm_fuse_link_in> lin((size_t)(nl > 0 ? nl : 1));
    for (int i = 0; i < count; ++i) { pin[(size_t)i].pair = pairs[i] ? pairs[i]->handle() : nullptr; pin[(size_t)i].d_points = nullptr; pin[(size_t)i].d_valid = nullptr; pin[(size_t)i].d_pose = nullptr; }
    for (int i = 0; i < nl; ++i) {
        lin[(size_t)i].d_index = indices[(size_t)i]; lin[(size_t)i].d_inlier = aouts[(size_t)i].d_inlier;
        lin[(size_t)i].d_sim = given ? reinterpret_cast<const float *>(given->p + 52 * (size_t)i) : aouts[(size_t)i].d_sim;
        lin[(size_t)i].d_err = aouts[(size_t)i].d_err; lin[(size_t)i].d_report = aouts[(size_t)i].d_report;
    }
    // the outputs in ONE block, every array at a multiple of 16 bytes
    const size_t k = (size_t)count;
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[11] = { 52 * k, 4 * k, 96 * k, 4 * N, 4 * (N + 1), 8 * N, 8 * N, 16 * N, N, 4 * N, 32 };
    size_t at[12];
    at[0] = 0;
    for (int q = 0; q < 11; ++q) at[q + 1] = at[q] + up(sizes[q] + 1);
    detail::DeviceBlock mem(at[11]);
    sfm_fuse_out o;
    o.d_frames = reinterpret_cast<float *>(mem.p + at[0]); o.d_root = reinterpret_cast<int32_t *>(mem.p + at[1]);
    o.d_cams = reinterpret_cast<float *>(mem.p + at[2]); o.d_track = reinterpret_cast<int32_t *>(mem.p + at[3]);
    o.d_track_offset = reinterpret_cast<int32_t *>(mem.p + at[4]); o.d_obs_cam = reinterpret_cast<int32_t *>(mem.p + at[5]);
    o.d_obs_record = reinterpret_cast<int32_t *>(mem.p + at[6]); o.d_points = reinterpret_cast<float *>(mem.p + at[7]);
    o.d_flags = reinterpret_cast<uint8_t *>(mem.p + at[8]); o.d_err = reinterpret_cast<float *>(mem.p + at[9]);
    o.d_counts = reinterpret_cast<int32_t *>(mem.p + at[10]);
    std::unique_ptr<detail::DeviceBlock> rep;              // the ring's report: allocated for fuse_ring alone
    if (report) {
        sfm_fuse_ring_params rp;
        sfm_fuse_ring_default_params(&rp);
        rp.fuse = fp;
        rep.reset(new detail::DeviceBlock(sizeof(sfm_fuse_ring_report) + 16));
        SFM_FACADE_CALL(sfm_fuse_ring(ctx, pin.data(), count, lin.data(), &rp, &o, reinterpret_cast<sfm_fuse_ring_report *>(rep->p)));
    } else SFM_FACADE_CALL(sfm_fuse_chain(ctx, pin.data(), count, lin.data(), &fp, &o));
    for (int i = 0; i < nl; ++i) r.links.push_back(scratch[(size_t)i]->download());        // (the first download waits for everything)
    int32_t counts[8];
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, counts, o.d_counts, sizeof(counts)));
    r.tracks = counts[0]; r.observations = counts[1]; r.refined = counts[2]; r.kept = counts[3]; r.segments = counts[4]; r.longest_track = counts[5];
    const size_t T = (size_t)r.tracks, M = (size_t)r.observations;
    std::vector<float> frames(13 * k), pts(4 * N);
    r.root.resize(k); r.cams.resize(24 * k); r.track.resize(N); r.track_offset.resize(T + 1); r.obs_cam.resize(M); r.obs_record.resize(M);
    r.points.resize(4 * T); r.flags.resize(T); r.err.resize(T);
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, frames.data(), o.d_frames, 52 * k));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.root.data(), o.d_root, 4 * k));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.cams.data(), o.d_cams, 96 * k));
    if (N) SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.track.data(), o.d_track, 4 * N));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.track_offset.data(), o.d_track_offset, 4 * (T + 1)));
    if (M) {
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.obs_cam.data(), o.d_obs_cam, 4 * M));
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.obs_record.data(), o.d_obs_record, 4 * M));
    }
    if (T) {
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, pts.data(), o.d_points, 16 * N));
        for (int c = 0; c < 4; ++c) std::copy(pts.begin() + (size_t)c * N, pts.begin() + (size_t)c * N + T, r.points.begin() + (size_t)c * T);
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.flags.data(), o.d_flags, T));
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.err.data(), o.d_err, 4 * T));
    }
    for (size_t i = 0; i < k; ++i) r.frames.push_back(Sim3::from(frames.data() + 13 * i));
    if (report) SFM_FACADE_CALL(sfm_copy_to_host(ctx, report, rep->p, sizeof(*report)));
    return r;
}
} // namespace detail

// A chain of `count` refined pairs, pair i + 1's first view being pair i's second, fused into tracks and one point per track
// (sfm_align_pairs over the count - 1 links, then sfm_fuse_chain): data[i] = the records pairs[i]'s fillXU took.  One wait at
// the end.  corrected_links: null, or 13 x (count - 1) floats the fusion reads in place of the measured links (the first
// count - 1 of ClosedRing::corrected: the chain of a closed ring); the links are aligned all the same, for their masks and
// errors, and FusedModel::links stays what the alignment measured.
inline FusedModel fuse_chain(Image_pair *const *pairs, SiftPoint *const *data, int count, int max_iterations = 5, float threshold_px = 4.0f,
                             const float *corrected_links = nullptr)
{
    return detail::fuse_links(pairs, data, count, max_iterations, threshold_px, corrected_links, nullptr);
}

// what fuse_ring returns: the model (links: all count of them; flags: also SFM_FUSE_SEAM_REFINED / SFM_FUSE_SEAM_KEPT for the tracks
// that cross the seam, which adjust_chain leaves alone) and the call's report
struct FusedRing {
    FusedModel model;
    sfm_fuse_ring_report report;
};

// A RING of `count` (>= 3) refined pairs fused (sfm_align_pairs over all count links, then sfm_fuse_ring): fuse_chain with the
// tracks that cross the seam joined.  corrected_links: 13 x count floats, ClosedRing::corrected -- the measured links of a real
// ring do not pass the call's closure gates (report.status is then SFM_RING_REJECTED and the model is fuse_chain's).
inline FusedRing fuse_ring(Image_pair *const *pairs, SiftPoint *const *data, int count, const float *corrected_links, int max_iterations = 5,
                           float threshold_px = 4.0f)
{
    FusedRing r;
    memset(&r.report, 0, sizeof(r.report));
    r.model = detail::fuse_links(pairs, data, count, max_iterations, threshold_px, corrected_links, &r.report);
    return r;
}

// what close_ring returns, in host memory
struct ClosedRing {
    std::vector<PairLink> links;        // count: the measured links as align_pairs gives them; link count - 1 closes the ring
    std::vector<float> corrected;       // 13 x count: the corrected links (s, R, t) as sfm_close_ring rounds them
    std::vector<Sim3> frames;           // count: the closed frames (the open ones unless report.status is SFM_RING_CLOSED)
    sfm_ring_report report;
};

// A ring of `count` (>= 3) refined pairs, pair i + 1 mod count's first view being pair i's second, closed (sfm_align_pairs over
// all count links, the last one carrying pair count - 1 onto pair 0, then sfm_close_ring): data[i] = the records pairs[i]'s fillXU
// took.  The first count - 1 corrected links go into fuse_chain.  One wait at the end.
inline ClosedRing close_ring(Image_pair *const *pairs, SiftPoint *const *data, int count, float threshold_px = 4.0f)
{
    ClosedRing r;
    sfm_ctx *ctx = sfm_facade::context();
    sfm_align_params ap;
    sfm_align_default_params(&ap);
    sfm_ring_params rp;
    sfm_ring_default_params(&rp);
    rp.threshold_px = threshold_px;
    std::vector<sfm_pair *> ha, hb;
    std::vector<std::unique_ptr<detail::AlignScratch>> scratch;
    std::vector<const int32_t *> indices;
    std::vector<sfm_align_out> aouts;
    std::vector<sfm_ring_link_in> lin;
    for (int i = 0; i < count; ++i) {
        Image_pair *b = pairs[(i + 1) % count];
        ha.push_back(pairs[i] ? pairs[i]->handle() : nullptr);
        hb.push_back(b ? b->handle() : nullptr);
        const int n = pairs[i] ? pairs[i]->numPoints() : 0;
        scratch.emplace_back(new detail::AlignScratch(n));
        SFM_FACADE_CALL(sfm_align_index_from_matches(ctx, reinterpret_cast<const sfm_sift_point *>(data[i]), n, 0.85f, 0.95f, scratch.back()->index()));
        indices.push_back(scratch.back()->index());
        aouts.push_back(scratch.back()->out());
        sfm_ring_link_in l;
        l.d_sim = aouts.back().d_sim; l.d_report = aouts.back().d_report;
        lin.push_back(l);
    }
    if (count > 0) SFM_FACADE_CALL(sfm_align_pairs(ha.data(), hb.data(), count, indices.data(), &ap, aouts.data()));
    const size_t k = (size_t)(count > 0 ? count : 0);
    detail::DeviceBlock mem(2 * (52 * k + 16) + sizeof(sfm_ring_report) + 16);
    sfm_ring_out o;
    o.d_links = reinterpret_cast<float *>(mem.p); o.d_frames = reinterpret_cast<float *>(mem.p + 52 * k + 16);
    o.d_seam_err = nullptr;
    o.d_report = reinterpret_cast<sfm_ring_report *>(mem.p + 2 * (52 * k + 16));
    sfm_fuse_pair_in last;
    last.pair = count > 0 && pairs[count - 1] ? pairs[count - 1]->handle() : nullptr;
    last.d_points = nullptr; last.d_valid = nullptr; last.d_pose = nullptr;
    SFM_FACADE_CALL(sfm_close_ring(ctx, lin.data(), count, &last, &rp, &o));
    for (int i = 0; i < count; ++i) r.links.push_back(scratch[(size_t)i]->download());      // (the first download waits for everything)
    std::vector<float> frames(13 * k);
    r.corrected.resize(13 * k);
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.corrected.data(), o.d_links, 52 * k));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, frames.data(), o.d_frames, 52 * k));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, &r.report, o.d_report, sizeof(r.report)));
    for (size_t i = 0; i < k; ++i) r.frames.push_back(Sim3::from(frames.data() + 13 * i));
    return r;
}

// what adjust_chain returns, in host memory
struct AdjustedChain {
    std::vector<float> cams;            // 24 x count, FusedModel::cams' layout: one camera per view inside a segment
    std::vector<float> points;          // 4 x T (leading dimension T)
    std::vector<uint8_t> used;          // T: the track took part
    std::vector<float> err;             // T: largest pixel error over the track's views under the returned cameras
    std::vector<sfm_adjust_chain_report> reports;    // count: filled at every segment's root
};

// One bundle adjustment per segment over every camera and every used track of a fused chain (sfm_adjust_chain): pairs, count:
// what fuse_chain took; model: what it returned.  The model is uploaded again (fuse_chain keeps nothing on the device); one
// wait at the end.
inline AdjustedChain adjust_chain(Image_pair *const *pairs, int count, const FusedModel &model, int max_iterations = 10, int max_track_views = 8)
{
    AdjustedChain r;
    if (count <= 0) return r;
    sfm_ctx *ctx = sfm_facade::context();
    sfm_adjust_chain_params p;
    sfm_adjust_chain_default_params(&p);
    p.max_iterations = max_iterations;
    p.max_track_views = max_track_views;
    std::vector<sfm_pair *> handles;
    size_t N = 0;
    for (int i = 0; i < count; ++i) { handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr); N += pairs[i] ? (size_t)pairs[i]->numPoints() : 0; }
    const size_t k = (size_t)count, T = (size_t)model.tracks, M = (size_t)model.observations;
    // inputs and outputs in ONE block, every array at a multiple of 16 bytes
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[13] = { 4 * k, 96 * k, 4 * (N + 1), 8 * N, 8 * N, 16 * N, N, 32, 96 * k, 16 * N, N, 4 * N, sizeof(sfm_adjust_chain_report) * k };
    size_t at[14];
    at[0] = 0;
    for (int q = 0; q < 13; ++q) at[q + 1] = at[q] + up(sizes[q] + 1);
    detail::DeviceBlock mem(at[13]);
    std::vector<float> pts(4 * N, 0.0f);
    for (int c = 0; c < 4; ++c) std::copy(model.points.begin() + (size_t)c * T, model.points.begin() + (size_t)c * T + T, pts.begin() + (size_t)c * N);
    const int32_t counts[8] = { model.tracks, model.observations, model.refined, model.kept, model.segments, model.longest_track, 0, 0 };
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[0], model.root.data(), 4 * k));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[1], model.cams.data(), 96 * k));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[2], model.track_offset.data(), 4 * (T + 1)));
    if (M) {
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[3], model.obs_cam.data(), 4 * M));
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[4], model.obs_record.data(), 4 * M));
    }
    if (N) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[5], pts.data(), 16 * N));
    if (T) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[6], model.flags.data(), T));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[7], counts, sizeof(counts)));
    sfm_adjust_chain_in in;
    in.pairs = handles.data();
    in.d_root = reinterpret_cast<const int32_t *>(mem.p + at[0]); in.d_cams = reinterpret_cast<const float *>(mem.p + at[1]);
    in.d_track_offset = reinterpret_cast<const int32_t *>(mem.p + at[2]); in.d_obs_cam = reinterpret_cast<const int32_t *>(mem.p + at[3]);
    in.d_obs_record = reinterpret_cast<const int32_t *>(mem.p + at[4]); in.d_points = reinterpret_cast<const float *>(mem.p + at[5]);
    in.d_flags = reinterpret_cast<const uint8_t *>(mem.p + at[6]); in.d_counts = reinterpret_cast<const int32_t *>(mem.p + at[7]);
    sfm_adjust_chain_out o;
    o.d_cams = reinterpret_cast<float *>(mem.p + at[8]); o.d_points = reinterpret_cast<float *>(mem.p + at[9]);
    o.d_used = reinterpret_cast<uint8_t *>(mem.p + at[10]); o.d_err = reinterpret_cast<float *>(mem.p + at[11]);
    o.d_reports = reinterpret_cast<sfm_adjust_chain_report *>(mem.p + at[12]);
    SFM_FACADE_CALL(sfm_adjust_chain(ctx, &in, count, &p, &o));
    r.cams.resize(24 * k); r.points.resize(4 * T); r.used.resize(T); r.err.resize(T); r.reports.resize(k);
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.cams.data(), o.d_cams, 96 * k));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.reports.data(), o.d_reports, sizeof(sfm_adjust_chain_report) * k));
    if (T) {
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, pts.data(), o.d_points, 16 * N));
        for (int c = 0; c < 4; ++c) std::copy(pts.begin() + (size_t)c * N, pts.begin() + (size_t)c * N + T, r.points.begin() + (size_t)c * T);
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.used.data(), o.d_used, T));
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.err.data(), o.d_err, 4 * T));
    }
    return r;
}

// what adjust_ring returns, in host memory
struct AdjustedRing {
    std::vector<float> cams;            // 24 x count, FusedModel::cams' layout: one camera per VIEW (pair count - 1's camera 2 is pair 0's camera 1)
    std::vector<float> points;          // 4 x T (leading dimension T)
    std::vector<uint8_t> used;          // T: the track took part (seam tracks included)
    std::vector<float> err;             // T: largest pixel error over the track's views under the returned cameras
    sfm_adjust_ring_report report;
};

// One bundle adjustment over a CLOSED ring, seam tracks included, view 0 fixed (sfm_adjust_ring): pairs, count: what fuse_ring
// took; ring: what it returned.  A ring that is not SFM_RING_CLOSED comes back as it went in (report.ring_status says so): adjust
// such a model by adjust_chain.  The model is uploaded again; one wait at the end.
inline AdjustedRing adjust_ring(Image_pair *const *pairs, int count, const FusedRing &ring, int max_iterations = 10, int max_track_views = 8)
{
    AdjustedRing r;
    memset(&r.report, 0, sizeof(r.report));
    const FusedModel &model = ring.model;
    sfm_ctx *ctx = sfm_facade::context();
    sfm_adjust_ring_params p;
    sfm_adjust_ring_default_params(&p);
    p.max_iterations = max_iterations;
    p.max_track_views = max_track_views;
    std::vector<sfm_pair *> handles;
    size_t N = 0;
    for (int i = 0; i < count; ++i) { handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr); N += pairs[i] ? (size_t)pairs[i]->numPoints() : 0; }
    const size_t k = (size_t)(count > 0 ? count : 0), T = (size_t)model.tracks, M = (size_t)model.observations;
    // inputs and outputs in ONE block, every array at a multiple of 16 bytes
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[14] = { 4 * k, 96 * k, 4 * (N + 1), 8 * N, 8 * N, 16 * N, N, 32, sizeof(sfm_fuse_ring_report), 96 * k, 16 * N, N, 4 * N,
                               sizeof(sfm_adjust_ring_report) };
    size_t at[15];
    at[0] = 0;
    for (int q = 0; q < 14; ++q) at[q + 1] = at[q] + up(sizes[q] + 1);
    detail::DeviceBlock mem(at[14]);
    std::vector<float> pts(4 * N, 0.0f);
    for (int c = 0; c < 4; ++c) std::copy(model.points.begin() + (size_t)c * T, model.points.begin() + (size_t)c * T + T, pts.begin() + (size_t)c * N);
    const int32_t counts[8] = { model.tracks, model.observations, model.refined, model.kept, model.segments, model.longest_track, 0, 0 };
    if (k) {
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[0], model.root.data(), 4 * k));
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[1], model.cams.data(), 96 * k));
    }
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[2], model.track_offset.data(), 4 * (T + 1)));
    if (M) {
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[3], model.obs_cam.data(), 4 * M));
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[4], model.obs_record.data(), 4 * M));
    }
    if (N) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[5], pts.data(), 16 * N));
    if (T) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[6], model.flags.data(), T));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[7], counts, sizeof(counts)));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[8], &ring.report, sizeof(ring.report)));
    sfm_adjust_ring_in in;
    in.pairs = handles.data();
    in.d_root = reinterpret_cast<const int32_t *>(mem.p + at[0]); in.d_cams = reinterpret_cast<const float *>(mem.p + at[1]);
    in.d_track_offset = reinterpret_cast<const int32_t *>(mem.p + at[2]); in.d_obs_cam = reinterpret_cast<const int32_t *>(mem.p + at[3]);
    in.d_obs_record = reinterpret_cast<const int32_t *>(mem.p + at[4]); in.d_points = reinterpret_cast<const float *>(mem.p + at[5]);
    in.d_flags = reinterpret_cast<const uint8_t *>(mem.p + at[6]); in.d_counts = reinterpret_cast<const int32_t *>(mem.p + at[7]);
    in.d_ring_report = reinterpret_cast<const sfm_fuse_ring_report *>(mem.p + at[8]);
    sfm_adjust_ring_out o;
    o.d_cams = reinterpret_cast<float *>(mem.p + at[9]); o.d_points = reinterpret_cast<float *>(mem.p + at[10]);
    o.d_used = reinterpret_cast<uint8_t *>(mem.p + at[11]); o.d_err = reinterpret_cast<float *>(mem.p + at[12]);
    o.d_report = reinterpret_cast<sfm_adjust_ring_report *>(mem.p + at[13]);
    SFM_FACADE_CALL(sfm_adjust_ring(ctx, &in, count, &p, &o));
    r.cams.resize(24 * k); r.points.resize(4 * T); r.used.resize(T); r.err.resize(T);
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.cams.data(), o.d_cams, 96 * k));
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, &r.report, o.d_report, sizeof(r.report)));
    if (T) {
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, pts.data(), o.d_points, 16 * N));
        for (int c = 0; c < 4; ++c) std::copy(pts.begin() + (size_t)c * N, pts.begin() + (size_t)c * N + T, r.points.begin() + (size_t)c * T);
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.used.data(), o.d_used, T));
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.err.data(), o.d_err, 4 * T));
    }
    return r;
}

// what intersect_tracks returns, in host memory
struct IntersectedTracks {
    std::vector<float> points;          // 4 x T (leading dimension T)
    std::vector<uint8_t> flags;         // T: SFM_FUSE_*, every track in the class it came in
    std::vector<float> err;             // T: largest pixel error over the track's views
    int32_t counts[8];                  // tracks, re-intersected, REFINED class, KEPT class, copied through, started from the linear
                                        // intersection, without an eligible start, promoted
};

// Every track of a fused model intersected over all its views under a camera table (sfm_intersect_tracks): pairs, count: what
// fuse_chain / fuse_ring took; model: what it returned; cams: 24 x count floats in FusedModel::cams' layout (an adjustment's cameras),
// null = the model's own; points: 4 x T, the columns to start from (an adjustment's points), null = the model's own; skip: T bytes
// (an adjustment's used flags: those tracks are copied through), or null.  The model is uploaded again; one wait at the end.
inline IntersectedTracks intersect_tracks(Image_pair *const *pairs, int count, const FusedModel &model, const float *cams = nullptr,
                                          const float *points = nullptr, const uint8_t *skip = nullptr, int max_iterations = 5,
                                          float threshold_px = 4.0f)
{
    IntersectedTracks r;
    memset(r.counts, 0, sizeof(r.counts));
    if (count <= 0) return r;
    sfm_ctx *ctx = sfm_facade::context();
    sfm_intersect_params p;
    sfm_intersect_default_params(&p);
    p.max_iterations = max_iterations;
    p.threshold_px = threshold_px;
    std::vector<sfm_pair *> handles;
    size_t N = 0;
    for (int i = 0; i < count; ++i) { handles.push_back(pairs[i] ? pairs[i]->handle() : nullptr); N += pairs[i] ? (size_t)pairs[i]->numPoints() : 0; }
    const size_t k = (size_t)count, T = (size_t)model.tracks, M = (size_t)model.observations;
    // inputs and outputs in ONE block, every array at a multiple of 16 bytes
    auto up = [](size_t b) { return (b + 15) / 16 * 16; };
    const size_t sizes[12] = { 96 * k, 4 * (N + 1), 8 * N, 8 * N, 16 * N, N, 32, N, 16 * N, N, 4 * N, 32 };
    size_t at[13];
    at[0] = 0;
    for (int q = 0; q < 12; ++q) at[q + 1] = at[q] + up(sizes[q] + 1);
    detail::DeviceBlock mem(at[12]);
    const float *src = points ? points : model.points.data();
    std::vector<float> pts(4 * N, 0.0f);
    for (int c = 0; c < 4; ++c) std::copy(src + (size_t)c * T, src + (size_t)c * T + T, pts.begin() + (size_t)c * N);
    const int32_t counts[8] = { model.tracks, model.observations, model.refined, model.kept, model.segments, model.longest_track, 0, 0 };
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[0], cams ? cams : model.cams.data(), 96 * k));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[1], model.track_offset.data(), 4 * (T + 1)));
    if (M) {
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[2], model.obs_cam.data(), 4 * M));
        SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[3], model.obs_record.data(), 4 * M));
    }
    if (N) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[4], pts.data(), 16 * N));
    if (T) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[5], model.flags.data(), T));
    SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[6], counts, sizeof(counts)));
    if (T && skip) SFM_FACADE_CALL(sfm_copy_to_device(ctx, mem.p + at[7], skip, T));
    sfm_intersect_in in;
    in.pairs = handles.data();
    in.d_cams = reinterpret_cast<const float *>(mem.p + at[0]); in.d_track_offset = reinterpret_cast<const int32_t *>(mem.p + at[1]);
    in.d_obs_cam = reinterpret_cast<const int32_t *>(mem.p + at[2]); in.d_obs_record = reinterpret_cast<const int32_t *>(mem.p + at[3]);
    in.d_points = reinterpret_cast<const float *>(mem.p + at[4]); in.d_flags = reinterpret_cast<const uint8_t *>(mem.p + at[5]);
    in.d_counts = reinterpret_cast<const int32_t *>(mem.p + at[6]);
    in.d_skip = skip ? reinterpret_cast<const uint8_t *>(mem.p + at[7]) : nullptr;
    sfm_intersect_out o;
    o.d_points = reinterpret_cast<float *>(mem.p + at[8]); o.d_flags = reinterpret_cast<uint8_t *>(mem.p + at[9]);
    o.d_err = reinterpret_cast<float *>(mem.p + at[10]); o.d_counts = reinterpret_cast<int32_t *>(mem.p + at[11]);
    SFM_FACADE_CALL(sfm_intersect_tracks(ctx, &in, count, &p, &o));
    r.points.resize(4 * T); r.flags.resize(T); r.err.resize(T);
    SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.counts, o.d_counts, sizeof(r.counts)));
    if (T) {
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, pts.data(), o.d_points, 16 * N));
        for (int c = 0; c < 4; ++c) std::copy(pts.begin() + (size_t)c * N, pts.begin() + (size_t)c * N + T, r.points.begin() + (size_t)c * T);
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.flags.data(), o.d_flags, T));
        SFM_FACADE_CALL(sfm_copy_to_host(ctx, r.err.data(), o.d_err, 4 * T));
    }
    return r;
}

} // namespace SfM

#endif
