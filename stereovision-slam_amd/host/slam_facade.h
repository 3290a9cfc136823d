// slam_facade.h — the reference's public classes, by name and signature, over the batched host
// pipeline (slam_host.h) with ONE stream: what a user of farhad-dalirani/StereoVision-SLAM links
// against instead of its Frontend / Backend / Dataset / VisualOdometry when the hot path moves to
// the GPU.  Same method names, argument meaning and return values:
//
//   Frontend   include/StereoVisionSLAM/frontend.h:36-44   SetMap SetBackend SetLoopClosure SetViewer
//                                                           SetCameras GetLastFrame GetStatus AddFrame
//   Backend    include/StereoVisionSLAM/backend.h:28-43    UpdateMap Stop PauseRequest IsPaused
//                                                           IsRunning Resume SetMap SetCameras
//   Dataset    src/dataset.cpp:11-138                      initialize (calib.txt -> 4 cameras, K *= 0.5,
//                                                           baseline = |K^-1 t|)  NextFrame  FrameById
//                                                           GetCamera GetDataDir GetLeftCamIndex
//   VisualOdometry  src/visual_odometry.cpp:24-224          initialize step run GetFrontendStatus
//                                                           saveSLAMOutputInFile
//   Map        include/StereoVisionSLAM/map.h               read-only views (keyframes, landmarks)
//   DenseReconstruction  src/dense_reconstruction.cpp:13-238  Initialize DenseReconstruct  (the second program,
//                                                           run_dense_reconstruction: keyframes.txt -> dense_map.pcd)
//
// Differences, all forced by the missing third-party libraries: cv::Mat becomes facade::Image (u8, one
// channel, or three in b, g, r order for the dense program's colour input), Sophus::SE3d becomes svs::SE3 (same 7 doubles), Frame::Ptr / Camera::Ptr stay shared_ptrs.
// The loop-closure and viewer objects of the reference are callbacks here (SetLoopClosure / SetViewer):
// they receive exactly what src/frontend.cpp:631-640 hands them, the new keyframe.  The backend
// "thread" is the pipeline's deterministic schedule: Backend::UpdateMap() from outside
// optimises at once.  The 1/2 INTER_NEAREST resize of Dataset::NextFrame (src/dataset.cpp:126-129)
// is not done on the host: frames keep their full resolution and the decimation is fused into the
// pyramid's level 0 on the device.
//
// Template over the kernel provider: the product instantiates HipKernels (kernels_hip.h); the test
// infrastructure instantiates the oracle's provider to test this file without a GPU.
#pragma once
#include <zlib.h>

#include <cstdio>
#include <fstream>
#include <functional>
#include <iomanip>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "slam_host.h"

namespace svs {
namespace facade {

struct SLAMException : std::runtime_error { using std::runtime_error::runtime_error; };   // slamexception.h

struct Image {                       // stand-in for cv::Mat CV_8UC1 (channels 1) / CV_8UC3 in b, g, r order (channels 3)
    int cols = 0, rows = 0;
    int channels = 1;
    std::vector<uint8_t> data;       // tight rows of cols * channels bytes
    bool empty() const { return data.empty(); }
};

// ---- image files: 8-bit PNG (grey, grey+alpha, RGB, RGBA; non-interlaced) through zlib, and binary PGM.
// cv::imread(path, IMREAD_GRAYSCALE): colour becomes grey by SVSLAM_GREY_FROM_RGB (include/svslam.h; the device conversion of
// the dense program's colour input uses the same definition).  cv::imread(path, IMREAD_COLOR): three channels b, g, r; a grey
// file is replicated into them, alpha is dropped.
enum ImreadModes { IMREAD_GRAYSCALE = 0, IMREAD_COLOR = 1 };
inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
inline bool read_png(const std::vector<uint8_t> &f, Image &img, bool colour = false)
{
    static const uint8_t sig[8] = { 0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a };
    if (f.size() < 33 || std::memcmp(f.data(), sig, 8) != 0) return false;
    size_t p = 8;
    uint32_t w = 0, h = 0;
    int depth = 0, ctype = 0, interlace = 0;
    std::vector<uint8_t> z;
    bool first = true;
    while (p + 12 <= f.size()) {
        const uint32_t len = be32(&f[p]);
        const char *ty = reinterpret_cast<const char *>(&f[p + 4]);
        if (p + 12 + (size_t)len > f.size()) return false;
        const uint8_t *d = &f[p + 8];
        const bool ihdr = !std::memcmp(ty, "IHDR", 4);
        if (first != ihdr) return false;                       // IHDR is the first chunk and appears once
        first = false;
        if (ihdr) {
            if (len != 13) return false;
            w = be32(d); h = be32(d + 4); depth = d[8]; ctype = d[9]; interlace = d[12];
        }
        else if (!std::memcmp(ty, "IDAT", 4)) z.insert(z.end(), d, d + len);
        else if (!std::memcmp(ty, "IEND", 4)) break;
        p += 12 + (size_t)len;
    }
    // a corrupt file yields an empty image (what cv::imread returns), never an oversized allocation
    if (!w || !h || w > 16384 || h > 16384 || depth != 8 || interlace != 0 || z.empty()) return false;
    const int ch = ctype == 0 ? 1 : ctype == 4 ? 2 : ctype == 2 ? 3 : ctype == 6 ? 4 : 0;
    if (!ch) return false;
    const size_t stride = (size_t)w * ch;
    std::vector<uint8_t> raw((stride + 1) * h);
    uLongf rawlen = (uLongf)raw.size();
    if (uncompress(raw.data(), &rawlen, z.data(), (uLong)z.size()) != Z_OK || rawlen != raw.size()) return false;
    std::vector<uint8_t> cur(stride), prev(stride, 0);
    const size_t oc = colour ? 3 : 1;
    img.cols = (int)w; img.rows = (int)h; img.channels = (int)oc; img.data.assign((size_t)w * h * oc, 0);
    for (uint32_t y = 0; y < h; ++y) {
        const uint8_t *r = &raw[(stride + 1) * y];
        const int ft = r[0];
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= (size_t)ch ? cur[i - ch] : 0, b = prev[i], c = i >= (size_t)ch ? prev[i - ch] : 0;
            int v = r[1 + i];
            if (ft == 1) v += a;
            else if (ft == 2) v += b;
            else if (ft == 3) v += (a + b) >> 1;
            else if (ft == 4) { const int pa = std::abs(b - c), pb = std::abs(a - c), pc = std::abs(a + b - 2 * c); v += (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c); }
            else if (ft != 0) return false;
            cur[i] = (uint8_t)v;
        }
        uint8_t *o = &img.data[(size_t)y * w * oc];
        if (colour) for (uint32_t x = 0; x < w; ++x) {
            const uint8_t *q = &cur[(size_t)x * ch];
            if (ch <= 2) o[3 * x] = o[3 * x + 1] = o[3 * x + 2] = q[0];
            else { o[3 * x] = q[2]; o[3 * x + 1] = q[1]; o[3 * x + 2] = q[0]; }       // the file holds r, g, b
        }
        else if (ch <= 2) for (uint32_t x = 0; x < w; ++x) o[x] = cur[(size_t)x * ch];
        else for (uint32_t x = 0; x < w; ++x) {       // cv::cvtColor RGB2GRAY
            const uint8_t *q = &cur[(size_t)x * ch];
            o[x] = (uint8_t)SVSLAM_GREY_FROM_RGB(q[0], q[1], q[2]);
        }
        prev.swap(cur);
    }
    return true;
}
inline bool read_pgm(const std::vector<uint8_t> &f, Image &img, bool colour = false)
{
    if (f.size() < 7 || f[0] != 'P' || f[1] != '5') return false;
    size_t p = 2;
    int vals[3], n = 0;
    while (n < 3 && p < f.size()) {
        while (p < f.size() && std::isspace(f[p])) ++p;
        if (p < f.size() && f[p] == '#') { while (p < f.size() && f[p] != '\n') ++p; continue; }
        int v = 0; bool any = false;
        while (p < f.size() && std::isdigit(f[p])) { v = v * 10 + (f[p] - '0'); ++p; any = true; }
        if (!any) return false;
        vals[n++] = v;
    }
    ++p;                                         // the single whitespace after maxval
    if (n < 3 || vals[2] != 255 || vals[0] <= 0 || vals[1] <= 0 || vals[0] > 16384 || vals[1] > 16384 ||
        p + (size_t)vals[0] * vals[1] > f.size()) return false;
    img.cols = vals[0]; img.rows = vals[1]; img.channels = colour ? 3 : 1;
    if (!colour) img.data.assign(f.begin() + (long)p, f.begin() + (long)p + (long)vals[0] * vals[1]);
    else {
        const size_t n = (size_t)vals[0] * (size_t)vals[1];
        img.data.resize(3 * n);
        for (size_t i = 0; i < n; ++i) img.data[3 * i] = img.data[3 * i + 1] = img.data[3 * i + 2] = f[p + i];
    }
    return true;
}
inline Image imread(const std::string &path, int flags = IMREAD_GRAYSCALE)     // empty image when the file is missing or not understood, like cv::imread
{
    const bool colour = flags == IMREAD_COLOR;
    Image img;
    std::ifstream in(path, std::ios::binary);
    if (!in) return img;
    std::vector<uint8_t> f((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    try {
        if (!read_png(f, img, colour) && !read_pgm(f, img, colour)) img = Image();
    } catch (const std::exception &) { img = Image(); }        // bad_alloc / length_error on a corrupt header
    return img;
}

// ---- Config (src/config.cpp): the scalar keys of an OpenCV FileStorage YAML
class ConfigFile {
public:
    bool Load(const std::string &path)
    {
        std::ifstream in(path);
        if (!in) return false;
        std::string line;
        while (std::getline(in, line)) {
            const size_t h = line.find('#');
            if (h != std::string::npos) line.erase(h);
            const size_t c = line.find(':');
            if (c == std::string::npos || (!line.empty() && line[0] == '%')) continue;
            auto trim = [](std::string s) { const size_t a = s.find_first_not_of(" \t\r"), b = s.find_last_not_of(" \t\r"); return a == std::string::npos ? std::string() : s.substr(a, b - a + 1); };
            std::string val = trim(line.substr(c + 1));
            if (val.size() >= 2 && (val.front() == '"' || val.front() == '\'') && val.back() == val.front())
                val = val.substr(1, val.size() - 2);           // cv::FileStorage accepts quoted strings
            kv_.emplace_back(trim(line.substr(0, c)), val);
        }
        return true;
    }
    std::string Str(const std::string &k, const std::string &def = "") const { for (auto &e : kv_) if (e.first == k) return e.second; return def; }
    double Num(const std::string &k, double def) const { const std::string s = Str(k); return s.empty() ? def : std::atof(s.c_str()); }
private:
    std::vector<std::pair<std::string, std::string>> kv_;
};

// ---- Camera (include/StereoVisionSLAM/camera.h)
class Camera : public svs::Camera {
public:
    typedef std::shared_ptr<Camera> Ptr;
    Camera() {}
    Camera(double fx_, double fy_, double cx_, double cy_, double baseline_, const SE3 &pose_)
    { fx = fx_; fy = fy_; cx = cx_; cy = cy_; baseline = baseline_; pose = pose_; }
};

// ---- Frame (include/StereoVisionSLAM/frame.h)
class Frame {
public:
    typedef std::shared_ptr<Frame> Ptr;
    unsigned long id_ = 0, keyframe_id_ = 0;
    bool is_keyframe_ = false;
    SE3 pose_;                                    // T_cw
    Image left_img_, right_img_;
    double time_stamp_ = 0;
    int n_features_ = 0, n_inliers_ = 0;          // filled by AddFrame (sizes of feature_left_ / inlier count)
    SE3 Pose() const { return pose_; }
    void SetPose(const SE3 &p) { pose_ = p; }
    static Ptr CreateFrame()                      // src/frame.cpp:22-28
    {
        static unsigned long factory_id = 0;
        Ptr f(new Frame());
        f->id_ = factory_id++;
        return f;
    }
};

// ---- Map (read-only mirror of include/StereoVisionSLAM/map.h for consumers of the facade)
struct KeyframeView { unsigned long id, keyframe_id; SE3 pose; bool active; };
struct LandmarkView { unsigned long id; double pos[3]; int observed_times; bool active; };
class Map {
public:
    typedef std::shared_ptr<Map> Ptr;
    std::function<std::vector<KeyframeView>()> keyframes_fn;
    std::function<std::vector<LandmarkView>()> landmarks_fn;
    std::vector<KeyframeView> GetAllKeyFrames() const { return keyframes_fn ? keyframes_fn() : std::vector<KeyframeView>(); }
    std::vector<KeyframeView> GetActiveKeyFrames() const { std::vector<KeyframeView> o; for (auto &k : GetAllKeyFrames()) if (k.active) o.push_back(k); return o; }
    std::vector<LandmarkView> GetAllMapPoints() const { return landmarks_fn ? landmarks_fn() : std::vector<LandmarkView>(); }
    std::vector<LandmarkView> GetActiveMapPoints() const { std::vector<LandmarkView> o; for (auto &l : GetAllMapPoints()) if (l.active) o.push_back(l); return o; }
};

using FrontendStatus = svs::FrontendStatus;

// ---- Backend (include/StereoVisionSLAM/backend.h:28-43): control handle of the pipeline's backend
class Backend {
public:
    typedef std::shared_ptr<Backend> Ptr;
    Backend() : running_(true), pause_request_(false) {}
    void UpdateMap() { if (running_ && !pause_request_ && optimize_now_) optimize_now_(); }
    void Stop() { running_ = false; apply(); }
    void PauseRequest() { pause_request_ = true; apply(); }
    bool IsPaused() const { return pause_request_; }       // the pipeline's backend stops at the request itself
    bool IsRunning() const { return running_; }
    void Resume() { pause_request_ = false; apply(); }
    void SetMap(Map::Ptr m) { map_ = m; }
    void SetCameras(Camera::Ptr l, Camera::Ptr r) { cam_left_ = l; cam_right_ = r; }
    // wiring (Frontend::SetBackend)
    std::function<void()> optimize_now_;
    std::function<void(bool)> set_enabled_;
    bool enabled() const { return running_ && !pause_request_; }
private:
    void apply() { if (set_enabled_) set_enabled_(enabled()); }
    bool running_, pause_request_;
    Map::Ptr map_;
    Camera::Ptr cam_left_, cam_right_;
};

// ---- Frontend (include/StereoVisionSLAM/frontend.h:36-44)
struct FrontendOptions {            // the hyper-parameters Frontend::Frontend() reads from Config (src/frontend.cpp:10-34)
    int num_features = 150, num_features_init = 50, num_features_tracking = 50, num_features_tracking_bad = 20;
    int num_features_needed_for_keyframe = 80;
    double max_triangulation_depth = 300.0;
    int num_active_keyframes = 10;
    double chi2_th = 5.991;
    int device = 0;
    // 1 (default): the stream's map — window, keyframe features, landmarks, observation counts — lives in device memory
    // and a keyframe is ONE chain of kernels (svslam_dmap_keyframe_batch), the configuration every throughput figure of
    // this library uses; 0: the host keeps it (rounds 1-2).  Same results bit for bit (tests/test_facade_kitti.py).
    // Not a key of the reference's config files: `device_map: 0` in the YAML (or this field) selects the host map.
    // A kernel provider without a device map (the CPU twin of the tests) ignores it.
    int device_map = 1;
    // Kernel shapes for ONE camera (svslam_set_low_latency): pose-only LM on four waves, a keyframe's local BA dealt over
    // up to 16 workgroups.  The facade is one stream by construction, like the reference's VisualOdometry::Step
    // (src/visual_odometry.cpp:109-156), so this is its default; `low_latency: 0` in the YAML (or this field) selects the
    // batch shapes (least total work — what a host that runs hundreds of streams through one context wants).  The two
    // shapes sum in different orders: results agree to rounding, each is deterministic.
    int low_latency = 1;
    // Parameter tolerance of the pose-only LM (svslam_set_pose_only_xtol, include/svslam.h): a round of EstimateCurrentPose ends at
    // a stationary point instead of spending the rest of its ten iterations on trials that move the pose by rounding noise.
    // `pose_xtol: 0` in the YAML (or this field) = g2o's schedule to the last trial (src/frontend.cpp:482-493 as written);
    // 1e-9 trades the last digits of the pose for a fifth of the kernel's time.
    double pose_xtol = 1e-12;
    // 1: every keyframe is described right after its step (Pipeline::DescribeNewKeyframes: BRIEF-256 at its non-outlier left
    // features, LoopClosure::ExtractKeypointsDescriptor) and keyframes keep their feature lists when they leave the window, so
    // that VerifyLoop(kf, cand, out) needs no descriptors from the caller.  `loop_descriptors: 1` in the YAML (or this field);
    // 0 (default): nothing is described, behaviour and memory as without the key.  Needs the host map (device_map: 0).
    // 2: the same with every feature described at its own angle and octave (Pipeline::DescribeNewKeyframesOriented,
    // svslam_orb_describe_batch): what the reference gets with the ORB detector.  With GFTT, 2 gives the bits of 1.
    int loop_descriptors = 0;
    // Frontend::DetectLoop's store of global descriptors: `loop_store_capacity` keyframes of `loop_descriptor_dim` floats (the
    // reference's vector has 1280); allocated at the first DetectLoop, never without it
    int loop_store_capacity = 4096, loop_descriptor_dim = 1280;
    // `loop_global_descriptor: <file>` in the YAML (or this field): a file written by gdesc.save (magic, version, layer table, prep,
    // parameters) that configures the network behind the global image descriptor at start (Pipeline::ConfigureGlobalDescriptor);
    // DetectLoop(out) then needs no vector from the caller and loop_descriptor_dim becomes the network's.  Empty (default): no network.
    std::string loop_global_descriptor;
    // `keypoint_feature_detector: ORB` of the reference's configuration (src/frontend.cpp:20-33): 1 = the ORB detector
    // (Pipeline::SetDetector, svslam_orb_detect_batch), which selects the host map; 0 (default, `GFTT`): goodFeaturesToTrack.
    // Any other value of the key throws.  ORB with loop_descriptors = 1 throws (one angle, level 0: wrong for ORB keypoints); 2 is its value.
    int detector = 0;
    static FrontendOptions FromConfig(const ConfigFile &c)
    {
        FrontendOptions o;
        o.device_map = (int)c.Num("device_map", o.device_map);
        o.low_latency = (int)c.Num("low_latency", o.low_latency);
        o.pose_xtol = c.Num("pose_xtol", o.pose_xtol);
        o.loop_descriptors = (int)c.Num("loop_descriptors", o.loop_descriptors);
        o.loop_store_capacity = (int)c.Num("loop_store_capacity", o.loop_store_capacity);
        o.loop_descriptor_dim = (int)c.Num("loop_descriptor_dim", o.loop_descriptor_dim);
        o.loop_global_descriptor = c.Str("loop_global_descriptor", "");
        o.num_features = (int)c.Num("num_features", o.num_features);
        o.num_features_init = (int)c.Num("num_features_init", o.num_features_init);
        o.num_features_tracking = (int)c.Num("num_features_tracking", o.num_features_tracking);
        o.num_features_tracking_bad = (int)c.Num("num_features_tracking_bad", o.num_features_tracking_bad);
        o.num_features_needed_for_keyframe = (int)c.Num("num_features_needed_for_keyframe", o.num_features_needed_for_keyframe);
        o.max_triangulation_depth = c.Num("max_triangulation_depth", o.max_triangulation_depth);
        o.num_active_keyframes = (int)c.Num("num_active_keyframes", o.num_active_keyframes);
        o.chi2_th = c.Num("chi2_th", o.chi2_th);
        const std::string det = c.Str("keypoint_feature_detector", "GFTT");
        if (det == "ORB") o.detector = 1;
        else if (det != "GFTT") throw SLAMException("Only the GFTT and ORB keypoint detectors are on the GPU path");
        if (o.loop_descriptors < 0 || o.loop_descriptors > 2) throw SLAMException("loop_descriptors: the values are 0 (none), 1 (one angle, level 0) and 2 (each keypoint's angle and octave)");
        if (o.detector == 1 && o.loop_descriptors == 1)
            throw SLAMException("keypoint_feature_detector: ORB with loop_descriptors: 1 is not supported: 1 describes every feature at one angle on level 0; use loop_descriptors: 2, which describes each at its keypoint's angle and octave");
        return o;
    }
};

// does the kernel provider offer a device-resident map (HipKernels::kHasDeviceMap)?  The CPU twin's provider does not.
template <class K> constexpr auto provider_has_device_map(int) -> decltype(K::kHasDeviceMap) { return K::kHasDeviceMap; }
template <class K> constexpr bool provider_has_device_map(long) { return false; }
// does it offer the descriptor kernel (HipKernels::brief_describe)?  The providers of the CPU twins do not.
template <class K> constexpr auto provider_has_brief(int) -> decltype(&K::brief_describe, true) { return true; }
template <class K> constexpr bool provider_has_brief(long) { return false; }
// does it offer the global-descriptor network (HipKernels::gdesc_describe)?
template <class K> constexpr auto provider_has_gdesc(int) -> decltype(&K::gdesc_describe, true) { return true; }
template <class K> constexpr bool provider_has_gdesc(long) { return false; }

// A file written by gdesc.save, little-endian: "SVGD", u32 version = 1, u32 nlayers, nlayers x 6 i32, i32 out_w, i32 out_h, 3 f32 mean,
// f32 scale, i64 workspace_bytes, i64 nparams, nparams f32.  Throws SLAMException on a file that is not one.
struct GlobalDescriptorFile {
    std::vector<svslam_gd_layer> layers;
    std::vector<float> params;
    svslam_gd_prep prep;
    explicit GlobalDescriptorFile(const std::string &path)
    {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw SLAMException("loop_global_descriptor: cannot open " + path);
        std::vector<char> raw((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        size_t o = 0;
        auto take = [&](void *dst, size_t n) {
            if (o + n > raw.size()) throw SLAMException("loop_global_descriptor: " + path + " is truncated");
            std::memcpy(dst, raw.data() + o, n); o += n;
        };
        char magic[4]; uint32_t ver = 0, n = 0;
        take(magic, 4); take(&ver, 4); take(&n, 4);
        if (std::memcmp(magic, "SVGD", 4) != 0 || ver != 1 || n > 4096) throw SLAMException("loop_global_descriptor: " + path + " is not a version-1 descriptor file");
        layers.resize(n);
        for (uint32_t i = 0; i < n; ++i) { int32_t v[6]; take(v, 24); layers[i] = svslam_gd_layer{ v[0], v[1], v[2], v[3], v[4], v[5] }; }
        int32_t wh[2]; float ms[4]; int64_t ws = 0, np = 0;
        take(wh, 8); take(ms, 16); take(&ws, 8); take(&np, 8);
        std::memset(&prep, 0, sizeof(prep));
        prep.out_w = wh[0]; prep.out_h = wh[1]; prep.mean[0] = ms[0]; prep.mean[1] = ms[1]; prep.mean[2] = ms[2]; prep.scale = ms[3];
        prep.workspace_bytes = (long long)ws;
        if (np < 0 || (uint64_t)np * 4 != raw.size() - o) throw SLAMException("loop_global_descriptor: " + path + " does not hold the parameters its header counts");
        params.resize((size_t)np);
        if (np) take(params.data(), (size_t)np * 4);
    }
};

template <class K>
class FrontendT {
public:
    typedef std::shared_ptr<FrontendT> Ptr;
    explicit FrontendT(const FrontendOptions &opt = FrontendOptions()) : opt_(opt) {}
    ~FrontendT() { unwire(); }                    // the shared Backend / Map handles may outlive the frontend
    FrontendT(const FrontendT &) = delete;
    FrontendT &operator=(const FrontendT &) = delete;
    void SetMap(Map::Ptr map) { if (map_) { map_->keyframes_fn = nullptr; map_->landmarks_fn = nullptr; } map_ = map; wire_map(); }
    // The pipeline is created at the first AddFrame with local BA compiled in; a backend handle may be attached,
    // replaced or removed at any time (a frontend without one runs without optimisation, src/frontend.cpp:618-622).
    void SetBackend(std::shared_ptr<Backend> backend)
    {
        if (backend_) { backend_->optimize_now_ = nullptr; backend_->set_enabled_ = nullptr; }
        backend_ = backend;
        wire_backend();
    }
    // the reference's LoopClosure::AddNewKeyFrame / Viewer::UpdateMap call sites (src/frontend.cpp:631-640)
    void SetLoopClosure(std::function<void(const Frame::Ptr &)> on_new_keyframe) { loopclosure_ = std::move(on_new_keyframe); }
    void SetViewer(std::function<void(const Frame::Ptr &)> on_frame) { viewer_ = std::move(on_frame); }
    void SetCameras(Camera::Ptr left, Camera::Ptr right) { camera_left_ = left; camera_right_ = right; }
    Frame::Ptr GetLastFrame() { return last_frame_; }
    FrontendStatus GetStatus() const { return status_; }

    // Update Frontend when new frame (src/frontend.cpp:690-721); true like the reference's Track()
    bool AddFrame(Frame::Ptr frame)
    {
        if (!frame || frame->left_img_.empty() || frame->right_img_.empty()) return false;
        if (!pipe_) create(frame->left_img_.cols, frame->left_img_.rows);
        if (frame->left_img_.cols != src_w_ || frame->left_img_.rows != src_h_ || frame->right_img_.cols != src_w_ ||
            frame->right_img_.rows != src_h_)
            throw SLAMException("frame size changed");
        current_frame_ = frame;
        const void *l = frame->left_img_.data.data(), *r = frame->right_img_.data.data();
        FrameResult res;
        pipe_->step(&l, &r, nullptr, 0, &res);
        frame->pose_ = SE3(res.pose);
        frame->is_keyframe_ = res.is_keyframe != 0;
        if (frame->is_keyframe_) frame->keyframe_id_ = (unsigned long)res.keyframe_id;
        frame->n_features_ = res.n_features; frame->n_inliers_ = res.n_inliers;
        status_ = (FrontendStatus)res.status;
        if (frame->is_keyframe_ && opt_.loop_descriptors) describe_new_keyframe();
        if (frame->is_keyframe_ && loopclosure_) loopclosure_(frame);
        if (viewer_) viewer_(frame);
        last_frame_ = current_frame_;
        return true;
    }
    Pipeline<K> *pipeline() { return pipe_.get(); }
    // what the reference's LoopClosure leaves on a keyframe after a confirmed loop (src/loopclosure.cpp:598-606), for a caller that
    // brings its own place recognition: keyframe kf_id saw the older keyframe loop_kf_id again, T_rel = T_kf * T_loop^-1 as measured
    bool AddLoopEdge(unsigned long kf_id, unsigned long loop_kf_id, const SE3 &T_rel)
    {
        return pipe_ && pipe_->AddLoopEdge(0, (long)kf_id, (long)loop_kf_id, T_rel);
    }
    // LoopClosure::KeypointMatchWithLoopCandid + CalculatePose (src/loopclosure.cpp:286-437) for keyframe kf_id against the older
    // keyframe cand_kf_id, for a caller that brings its own place recognition and 256-bit descriptors: descriptors [n][32] of both
    // keyframes with desc_feat_indx (descriptor row -> index in feature_left_).  An ACCEPTED result is recorded like AddLoopEdge.
    // False: refused (pipeline()->last_error()), nothing done.  LocalFusion is the caller's: the result carries what it needs.
    bool VerifyLoop(unsigned long kf_id, unsigned long cand_kf_id, int nq, const uint8_t *desc_q, const int *feat_q, int nc,
                    const uint8_t *desc_c, const int *feat_c, const svslam_loop_params &params, typename Pipeline<K>::LoopResult *out)
    {
        if (!pipe_) return false;
        std::vector<typename Pipeline<K>::LoopResult> res;
        if (!pipe_->VerifyLoops({ typename Pipeline<K>::LoopQuery{ 0, (long)kf_id, (long)cand_kf_id, nq, desc_q, nq, feat_q, nc, desc_c, nc, feat_c } }, params, &res))
            return false;
        if (out) *out = res[0];
        return true;
    }
    // the same on the descriptors stored for both keyframes (`loop_descriptors: 1`); false also for a keyframe that was never described
    bool VerifyLoop(unsigned long kf_id, unsigned long cand_kf_id, const svslam_loop_params &params, typename Pipeline<K>::LoopResult *out)
    {
        if (!pipe_) return false;
        std::vector<typename Pipeline<K>::LoopResult> res;
        if (!pipe_->VerifyLoopsStored({ typename Pipeline<K>::LoopPair{ 0, (long)kf_id, (long)cand_kf_id } }, params, &res)) return false;
        if (out) *out = res[0];
        return true;
    }
    // LoopClosure::AddNewKeyFrame and one turn of LoopClosurePipeline (src/loopclosure.cpp:182-198, :801-872) for the keyframe the
    // last AddFrame made: Pipeline::DetectLoops on stream 0 with the caller's global descriptor of `loop_descriptor_dim` floats
    // (the reference's MobileNetV2 vector; the network is not part of this project).  The store is configured at the first call:
    // `loop_store_capacity` keyframes (default 4096).  Needs `loop_descriptors: 1`.  out->is_keyframe is false when the last frame
    // made no keyframe or it was handled already.  LocalFusion stays the caller's: out->loop carries what it needs.
    bool DetectLoop(const float *vec, const typename Pipeline<K>::LoopDetectParams &params, typename Pipeline<K>::LoopDetection *out)
    {
        if (!pipe_) return false;
        if (!opt_.loop_descriptors) throw SLAMException("DetectLoop needs loop_descriptors: 1 in the configuration");
        if (!loop_store_ready_) {
            if (!pipe_->ConfigureLoopStore(opt_.loop_store_capacity, opt_.loop_descriptor_dim)) return false;
            loop_store_ready_ = true;
        }
        std::vector<typename Pipeline<K>::LoopDetection> res;
        if (!pipe_->DetectLoops(vec, params, &res)) return false;
        if (out) *out = res[0];
        return true;
    }
    // the same with the vector computed by the network of `loop_global_descriptor` (LoopClosure::ExtractFeatureVec on the keyframe's
    // left image): a loop is closed from the frames alone.  Throws without the key, the way DetectLoop does without `loop_descriptors`.
    bool DetectLoop(const typename Pipeline<K>::LoopDetectParams &params, typename Pipeline<K>::LoopDetection *out)
    {
        if (!pipe_) return false;
        if (opt_.loop_global_descriptor.empty()) throw SLAMException("DetectLoop without a vector needs loop_global_descriptor: <file> in the configuration");
        return DetectLoop(nullptr, params, out);
    }
    K *kernels() { return kernels_.get(); }
    bool LowLatency() const { return opt_.low_latency != 0; }

private:
    // (a function of its own so that a provider without the kernel never instantiates Pipeline::DescribeNewKeyframes)
    void describe_new_keyframe()
    {
        if (opt_.loop_descriptors == 2) {
            if constexpr (provider_has_orb_describe<K>(0)) {
                if (!pipe_->DescribeNewKeyframesOriented()) throw SLAMException(pipe_->last_error());
            } else {
                throw SLAMException("loop_descriptors: 2: this kernel provider has no oriented descriptors");
            }
        } else if constexpr (provider_has_brief<K>(0)) {
            if (!pipe_->DescribeNewKeyframes()) throw SLAMException(pipe_->last_error());
        } else {
            throw SLAMException("loop_descriptors: this kernel provider has no descriptor kernel");
        }
    }
    // (a function of its own so that a provider without the kernels never instantiates Pipeline::ConfigureGlobalDescriptor)
    void configure_global_descriptor()
    {
        if constexpr (provider_has_gdesc<K>(0)) {
            const GlobalDescriptorFile F(opt_.loop_global_descriptor);
            if (!pipe_->ConfigureGlobalDescriptor((int)F.layers.size(), F.layers.data(), F.params.data(), (long long)F.params.size(), &F.prep))
                throw SLAMException(pipe_->last_error());
            opt_.loop_descriptor_dim = pipe_->GlobalDescriptorDim();
        } else {
            throw SLAMException("loop_global_descriptor: this kernel provider has no descriptor network");
        }
    }
    void create(int w, int h)
    {
        if (!camera_left_ || !camera_right_) throw SLAMException("Frontend: SetCameras before the first AddFrame");
        src_w_ = w; src_h_ = h;
        // Dataset halves K (src/dataset.cpp:73); the images arrive at full resolution and are halved on the device
        const int dw = (int)std::nearbyint(w * 0.5), dh = (int)std::nearbyint(h * 0.5);
        Config cfg;
        cfg.num_features = opt_.num_features; cfg.num_features_init = opt_.num_features_init;
        cfg.num_features_tracking = opt_.num_features_tracking; cfg.num_features_tracking_bad = opt_.num_features_tracking_bad;
        cfg.num_features_needed_for_keyframe = opt_.num_features_needed_for_keyframe;
        cfg.max_triangulation_depth = opt_.max_triangulation_depth;
        cfg.num_active_keyframes = opt_.num_active_keyframes; cfg.chi2_th = opt_.chi2_th;
        cfg.backend_on = 1;                        // gated by SetBackendEnabled: see SetBackend
        cfg.width = dw; cfg.height = dh; cfg.src_width = w; cfg.src_height = h;
        if (opt_.loop_descriptors < 0 || opt_.loop_descriptors > 2) throw SLAMException("loop_descriptors: the values are 0 (none), 1 (one angle, level 0) and 2 (each keypoint's angle and octave)");
        if (opt_.detector == 1 && opt_.loop_descriptors == 1)
            throw SLAMException("keypoint_feature_detector: ORB with loop_descriptors: 1 is not supported: 1 describes every feature at one angle on level 0; use loop_descriptors: 2, which describes each at its keypoint's angle and octave");
        const bool dmap = opt_.device_map != 0 && provider_has_device_map<K>(0) && cfg.num_active_keyframes + 1 <= 12 && opt_.detector == 0;
        cfg.resident_track = dmap ? 1 : 0;         // host map: the host keeps the feature lists; device map: nothing per feature on the host
        cfg.device_map = dmap ? 1 : 0;
        cfg.cam_l = *camera_left_; cfg.cam_r = *camera_right_;
        cfg.max_pts = 512; cfg.max_kf = cfg.num_active_keyframes + 1; cfg.max_lm = 4096; cfg.max_obs = 16384;
        svslam_limits lim;
        std::memset(&lim, 0, sizeof(lim));
        lim.device = opt_.device; lim.width = dw; lim.height = dh; lim.max_slots = 3; lim.max_jobs = 2;
        lim.max_pts = cfg.max_pts; lim.max_corners = cfg.num_features;
        lim.max_kf = cfg.max_kf; lim.max_lm = cfg.max_lm; lim.max_obs = cfg.max_obs;
        lim.max_streams = dmap ? 1 : 0; lim.device_map = dmap ? 1 : 0;
        kernels_.reset(new K(lim));
        if (kernels_->set_source_size(w, h) != 0) throw SLAMException(std::string("source size: ") + kernels_->last_error());
        if (kernels_->set_low_latency(opt_.low_latency ? 1 : 0) != 0) throw SLAMException(std::string("low-latency shapes: ") + kernels_->last_error());
        if (kernels_->set_pose_only_xtol(opt_.pose_xtol) != 0) throw SLAMException(std::string("pose_xtol: ") + kernels_->last_error());
        pipe_.reset(new Pipeline<K>(cfg, *kernels_, 1, 1));
        if (opt_.detector != 0 && !pipe_->SetDetector(opt_.detector)) {
            const std::string why = pipe_->last_error();        // no pipeline is left behind that would detect with GFTT instead
            pipe_.reset(); kernels_.reset();
            throw SLAMException(why);
        }
        if (opt_.loop_descriptors) pipe_->SetKeepKeyframeFeatures(true);
        if (!opt_.loop_global_descriptor.empty()) configure_global_descriptor();
        wire_backend(); wire_map();
    }
    void unwire()
    {
        if (backend_) { backend_->optimize_now_ = nullptr; backend_->set_enabled_ = nullptr; }
        if (map_) { map_->keyframes_fn = nullptr; map_->landmarks_fn = nullptr; }
    }
    void wire_backend()
    {
        if (!backend_) { if (pipe_) pipe_->SetBackendEnabled(false); return; }
        backend_->optimize_now_ = [this]() { if (pipe_) pipe_->OptimizeNow(); };
        backend_->set_enabled_ = [this](bool on) { if (pipe_) pipe_->SetBackendEnabled(on); };
        if (pipe_) pipe_->SetBackendEnabled(backend_->enabled());
    }
    void wire_map()
    {
        if (!map_) return;
        map_->keyframes_fn = [this]() {
            std::vector<KeyframeView> o;
            if (!pipe_) return o;
            auto &m = pipe_->stream(0).map;
            for (const svs::Frame *f : m.keyframes_) {
                bool act = false;
                for (const svs::Frame *a : m.active_keyframes_) act |= (a == f);
                o.push_back(KeyframeView{ (unsigned long)f->id, (unsigned long)f->keyframe_id, f->pose, act });
            }
            return o;
        };
        map_->landmarks_fn = [this]() {
            std::vector<LandmarkView> o;
            if (!pipe_) return o;
            for (const svs::LandmarkRecord &p : pipe_->AllLandmarks(0))
                o.push_back(LandmarkView{ (unsigned long)p.id, { p.pos[0], p.pos[1], p.pos[2] }, p.observed_times, p.active });
            return o;
        };
    }
    FrontendOptions opt_;
    FrontendStatus status_ = FrontendStatus::INITING;
    Frame::Ptr current_frame_, last_frame_;
    Camera::Ptr camera_left_, camera_right_;
    Map::Ptr map_;
    std::shared_ptr<Backend> backend_;
    std::function<void(const Frame::Ptr &)> loopclosure_, viewer_;
    std::unique_ptr<K> kernels_;
    std::unique_ptr<Pipeline<K>> pipe_;
    bool loop_store_ready_ = false;
    int src_w_ = 0, src_h_ = 0;
};

// ---- Dataset (src/dataset.cpp)
class Dataset {
public:
    typedef std::shared_ptr<Dataset> Ptr;
    // color_input: read with IMREAD_COLOR (src/dataset.cpp reads is_color_input from the config); only the dense program asks for it
    explicit Dataset(const std::string &dataset_path, int left_cam_index = 0, int right_cam_index = 1, bool color_input = false)
        : dataset_path_(dataset_path), left_cam_index_(left_cam_index), right_cam_index_(right_cam_index), color_input_(color_input) {}

    bool initialize()                             // :24-86
    {
        std::ifstream fin(dataset_path_ + "/calib.txt");
        if (!fin) throw SLAMException("Cannot open KITTI camera parameters file (calib.txt).");
        cameras_.clear();
        for (int i = 0; i < 4; ++i) {
            char cam_name[3];
            fin >> cam_name[0] >> cam_name[1] >> cam_name[2];
            double pr[12];
            for (int j = 0; j < 12; ++j) fin >> pr[j];
            if (!fin) throw SLAMException("calib.txt: expected four 3x4 projection matrices");
            // rectified: P = [K | K t]  ->  t = K^-1 (p03, p13, p23); K is upper triangular
            const double fx = pr[0], sk = pr[1], cx = pr[2], fy = pr[5], cy = pr[6], k22 = pr[10];
            const double b2 = pr[11] / k22;
            const double b1 = (pr[7] - cy * b2) / fy;
            const double b0 = (pr[3] - sk * b1 - cx * b2) / fx;
            const double baseline = std::sqrt(b0 * b0 + b1 * b1 + b2 * b2);
            SE3 pose;
            pose.v[4] = b0; pose.v[5] = b1; pose.v[6] = b2;
            // K *= 0.5: the pipeline works on the images down-sampled by two (:73)
            cameras_.push_back(Camera::Ptr(new Camera(0.5 * fx, 0.5 * fy, 0.5 * cx, 0.5 * cy, baseline, pose)));
        }
        current_image_index_ = 0;
        return true;
    }
    Camera::Ptr GetCamera(int camera_id) const { return cameras_.at((size_t)camera_id); }
    std::string GetDataDir() const { return dataset_path_; }
    int GetLeftCamIndex() const { return left_cam_index_; }

    Frame::Ptr NextFrame()                        // :104-138 (the resize happens on the device, see the header)
    {
        Frame::Ptr f = FrameById((unsigned long)current_image_index_);
        if (f) ++current_image_index_;
        return f;
    }
    Frame::Ptr FrameById(unsigned long frame_id)  // :140-176
    {
        Image l = load(left_cam_index_, frame_id), r = load(right_cam_index_, frame_id);
        if (l.empty() || r.empty()) return nullptr;
        Frame::Ptr f = Frame::CreateFrame();
        f->left_img_ = std::move(l); f->right_img_ = std::move(r);
        return f;
    }

private:
    Image load(int cam, unsigned long id) const
    {
        std::ostringstream base;
        base << dataset_path_ << "/image_" << cam << "/" << std::setw(6) << std::setfill('0') << id;
        const int flags = color_input_ ? IMREAD_COLOR : IMREAD_GRAYSCALE;
        Image img = imread(base.str() + ".png", flags);
        if (img.empty()) img = imread(base.str() + ".pgm", flags);
        return img;
    }
    std::string dataset_path_;
    int left_cam_index_, right_cam_index_;
    bool color_input_ = false;
    std::vector<Camera::Ptr> cameras_;
    int current_image_index_ = 0;
};

// ---- VisualOdometry (src/visual_odometry.cpp): the wiring of the classes above
template <class K>
class VisualOdometryT {
public:
    explicit VisualOdometryT(const std::string &config_file_path) : config_file_path_(config_file_path) {}
    bool initialize()                             // :24-107
    {
        if (!config_.Load(config_file_path_)) return false;
        dataset_.reset(new Dataset(config_.Str("dataset_dir"), (int)config_.Num("left_cam_index", 0), (int)config_.Num("right_cam_index", 1)));
        if (!dataset_->initialize()) return false;
        frontend_.reset(new FrontendT<K>(FrontendOptions::FromConfig(config_)));
        map_.reset(new Map());
        if ((int)config_.Num("backend_on", 1) != 0) backend_.reset(new Backend());
        frontend_->SetMap(map_);
        frontend_->SetBackend(backend_);
        frontend_->SetCameras(dataset_->GetCamera(0), dataset_->GetCamera(1));   // src/visual_odometry.cpp:73: always cameras 0 / 1; only the image folders follow left/right_cam_index
        if (backend_) { backend_->SetMap(map_); backend_->SetCameras(dataset_->GetCamera(0), dataset_->GetCamera(1)); }
        return true;
    }
    bool step()                                   // :109-146
    {
        Frame::Ptr f = dataset_->NextFrame();
        if (!f) return false;
        return frontend_->AddFrame(f);
    }
    void run()                                    // :148-180
    {
        while (step()) {}
        if (backend_) backend_->Stop();
        if (!Stop())        // refused (the map lives on the device): say so, the outputs below are the uncorrected ones
            std::fprintf(stderr, "VisualOdometry: global pose-graph optimisation not run: %s\n", frontend_->pipeline()->last_error().c_str());
        saveSLAMOutputInFile();
    }
    // LoopClosure::Stop() (src/visual_odometry.cpp:174-190, src/loopclosure.cpp:66-82): with global_pose_graph_optimization >= 1 one
    // pose-graph optimisation over the whole run before the outputs are written.  False: the optimisation was refused
    // (device-resident map); the outputs are then written uncorrected.
    bool Stop()
    {
        if ((int)config_.Num("global_pose_graph_optimization", 0) < 1 || !frontend_->pipeline()) return true;
        return frontend_->pipeline()->PoseGraphOptimization({ 0 });
    }
    bool AddLoopEdge(unsigned long kf_id, unsigned long loop_kf_id, const SE3 &T_rel) { return frontend_->AddLoopEdge(kf_id, loop_kf_id, T_rel); }
    // Frontend::VerifyLoop with the thresholds of the configuration file (the keys LoopClosure reads, src/loopclosure.cpp:26-36, in
    // their spelling) and the reference's constants of solvePnPRansac (:381: 100 iterations, 5.991 px)
    bool VerifyLoop(unsigned long kf_id, unsigned long cand_kf_id, int nq, const uint8_t *desc_q, const int *feat_q, int nc,
                    const uint8_t *desc_c, const int *feat_c, typename Pipeline<K>::LoopResult *out, unsigned seed = 0)
    {
        return frontend_->VerifyLoop(kf_id, cand_kf_id, nq, desc_q, feat_q, nc, desc_c, feat_c, loop_params(seed), out);
    }
    svslam_loop_params loop_params(unsigned seed) const
    {
        svslam_loop_params p;
        std::memset(&p, 0, sizeof(p));
        p.min_matches = (int)config_.Num("min_num_acceptable_keypoint_match", 20);
        p.ransac_iters = 100; p.reproj_px = 5.991; p.seed = seed;
        p.max_pose_distance = config_.Num("max_pose_distance_between_loop_keyframes", 20);
        p.min_pose_difference = config_.Num("min_pose_differnece_between_old_new", 1);
        p.max_pose_difference = config_.Num("max_pose_differnece_between_old_new", 50);
        return p;
    }
    // the same on the descriptors stored for both keyframes (`loop_descriptors: 1` in the configuration file)
    bool VerifyLoop(unsigned long kf_id, unsigned long cand_kf_id, typename Pipeline<K>::LoopResult *out, unsigned seed = 0)
    {
        return frontend_->VerifyLoop(kf_id, cand_kf_id, loop_params(seed), out);
    }
    // Frontend::DetectLoop with the thresholds of the configuration file, in the reference's spelling (src/loopclosure.cpp:26-36):
    // potential_loop_weak_threshold, potential_loop_strong_threshold, max_num_weak_threshold, keyframes_to_ignore_after_loop, the
    // keys of loop_params; the gap of 20 keyframes is :244's literal unless `loop_min_keyframe_gap` (a key of this project) says otherwise.  Call it after an AddFrame that made a keyframe.
    bool DetectLoop(const float *vec, typename Pipeline<K>::LoopDetection *out, unsigned seed = 0)
    {
        typename Pipeline<K>::LoopDetectParams p;
        p.cand.weak = (float)config_.Num("potential_loop_weak_threshold", 0.93);
        p.cand.strong = (float)config_.Num("potential_loop_strong_threshold", 0.95);
        p.cand.max_num_weak = (int)config_.Num("max_num_weak_threshold", 3);
        p.cand.min_gap = (int)config_.Num("loop_min_keyframe_gap", 20);
        p.verify = loop_params(seed);
        p.keyframes_to_ignore_after_loop = (long)config_.Num("keyframes_to_ignore_after_loop", 5);
        return vec ? frontend_->DetectLoop(vec, p, out) : frontend_->DetectLoop(p, out);
    }
    // the same from the frames alone: the vector is the configured network's (`loop_global_descriptor: <file>`); throws without the key
    bool DetectLoop(typename Pipeline<K>::LoopDetection *out, unsigned seed = 0) { return DetectLoop(nullptr, out, seed); }
    FrontendStatus GetFrontendStatus() const { return frontend_->GetStatus(); }
    // keyframes.txt + landmarks.pcd under output_dir (:198-310; the reference adds a time-stamped folder)
    bool saveSLAMOutputInFile(const std::string &dir_override = "")
    {
        const std::string dir = dir_override.empty() ? config_.Str("output_dir", ".") : dir_override;
        if (!frontend_->pipeline()) return false;
        frontend_->pipeline()->Flush();
        return frontend_->pipeline()->SaveOutputs(0, dir, dataset_->GetDataDir(), dataset_->GetLeftCamIndex());
    }
    std::shared_ptr<FrontendT<K>> frontend() { return frontend_; }
    std::shared_ptr<Backend> backend() { return backend_; }
    Map::Ptr map() { return map_; }
    Dataset::Ptr dataset() { return dataset_; }

private:
    std::string config_file_path_;
    ConfigFile config_;
    Dataset::Ptr dataset_;
    std::shared_ptr<FrontendT<K>> frontend_;
    std::shared_ptr<Backend> backend_;
    Map::Ptr map_;
};

// ---- DenseReconstruction (src/dense_reconstruction.cpp, include/StereoVisionSLAM/dense_reconstruction.h)
// Reads the dense config (slam_output_dir = the keyframes.txt VisualOdometry::saveSLAMOutputInFile wrote, left_cam_index,
// right_cam_index, output_dir), runs cv::StereoBM(128, 15) and the back-projection of every keyframe on the device
// (svslam_dense_cloud_batch, several keyframes per call) and writes output_dir/dense_map.pcd.
// Colour: with `is_color_input: 1` in the dense config — what every dense config of the reference says — the images
// are read IMREAD_COLOR, the grey images of the matcher are made on the device (svslam_pyramid_bgr_batch), the left image stays
// there as a colour plane and every point comes back with its b, g, r (svslam_dense_cloud_bgr_batch); the colours pass through the
// keep masks, the merge, both filters and the writer.  With 0 (this facade's default) the reader is greyscale and r = g = b = the
// grey value of the left pixel.
// Differences from the reference, all stated in DESIGN 9: PCL's StatisticalOutlierRemoval (k = 50, once per keyframe cloud and once on the merge) and the
// 2 cm VoxelGrid (:175-209) run only with `cloud_filters: 1` in the dense config (svslam_cloud_sor_batch, svslam_cloud_voxel_grid;
// their contract is tests/ref_cloud_filters.py) — the default 0 writes the unfiltered merge of the keyframe clouds in keyframe
// order, as before the filters existed; the file goes to output_dir itself, not into a
// time-stamped folder below it; as everywhere in this facade the 1/2 decimation of Dataset::FrameById happens on the device.
struct DenseKeyframe { unsigned long image_id; SE3 T_cw; };

// keyframes_poses_.push_back(Sophus::SE3f(T)) ... .cast<double>() (src/dense_reconstruction.cpp:59-72, :160): the twelve numbers
// of a keyframes.txt record are FLOATS; SE3f's constructor turns the rotation block into a quaternion IN FLOAT (Eigen's
// matrix-to-quaternion branches: trace > 0, else the largest diagonal entry), cast<double>() widens it and SO3d's
// constructor normalises it in double; the translation is widened.  Plain + - * / sqrt on floats, then on doubles, so a
// restatement in another language gives the same bits (only Eigen's summation order inside normalize() is not pinned).
inline SE3 se3_from_float_rows(const float m[12])
{
    const float R[3][3] = { { m[0], m[1], m[2] }, { m[4], m[5], m[6] }, { m[8], m[9], m[10] } };
    float q[4];                                    // x y z w
    float t = R[0][0] + R[1][1] + R[2][2];
    if (t > 0.f) {
        t = std::sqrt(t + 1.0f);
        q[3] = 0.5f * t;
        t = 0.5f / t;
        q[0] = (R[2][1] - R[1][2]) * t; q[1] = (R[0][2] - R[2][0]) * t; q[2] = (R[1][0] - R[0][1]) * t;
    } else {
        int i = 0;
        if (R[1][1] > R[0][0]) i = 1;
        if (R[2][2] > R[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0f);
        q[i] = 0.5f * t;
        t = 0.5f / t;
        q[3] = (R[k][j] - R[j][k]) * t; q[j] = (R[j][i] + R[i][j]) * t; q[k] = (R[k][i] + R[i][k]) * t;
    }
    const double qd[4] = { q[0], q[1], q[2], q[3] };
    const double n = std::sqrt(qd[0] * qd[0] + qd[1] * qd[1] + qd[2] * qd[2] + qd[3] * qd[3]);
    SE3 T;
    for (int i = 0; i < 4; ++i) T.v[i] = qd[i] / n;
    T.v[4] = m[3]; T.v[5] = m[7]; T.v[6] = m[11];
    return T;
}

template <class K>
class DenseReconstructionT {
public:
    explicit DenseReconstructionT(const std::string &config_file_path) : config_file_path_(config_file_path) {}

    void Initialize()                             // :18-90
    {
        if (!config_.Load(config_file_path_)) throw SLAMException("Can not open the dense reconstruction config file.");
        slam_output_dir_ = config_.Str("slam_output_dir");
        left_cam_index_ = (int)config_.Num("left_cam_index", 0);
        right_cam_index_ = (int)config_.Num("right_cam_index", 1);
        std::ifstream slam_fp(slam_output_dir_);
        if (!slam_fp) throw SLAMException("Can not open SLAM pipeline's output file.");
        slam_fp >> data_sequence_path_;
        slam_fp >> left_camera_index_in_slam_;
        keyframes_.clear();
        while (!slam_fp.eof()) {
            unsigned long image_id;
            slam_fp >> image_id;
            if (slam_fp.fail()) break;
            float m[12];
            bool ok = true;
            for (int i = 0; i < 12 && ok; ++i) { slam_fp >> m[i]; ok = !slam_fp.fail(); }        // parsed as float, like slam_fp >> T(i, j)
            if (!ok) break;
            keyframes_.push_back(DenseKeyframe{ image_id, se3_from_float_rows(m) });
        }
        color_input_ = (int)config_.Num("is_color_input", 0) != 0;
        dataset_.reset(new Dataset(data_sequence_path_, left_cam_index_, right_cam_index_, color_input_));
        if (!dataset_->initialize()) throw SLAMException("Cannot initialize object to read dataset.");
        params_.num_disparities = num_disparities_; params_.block_size = blockSize_;
        params_.pre_filter_cap = 31; params_.texture_threshold = 10; params_.uniqueness_ratio = 15; params_.reserved = 0;
        cloud_filters_ = (int)config_.Num("cloud_filters", 0) != 0;
        xyz_.clear(); bgr_.clear();
    }

    void DenseReconstruct()                       // :92-238
    {
        if (!dataset_) throw SLAMException("DenseReconstruction: Initialize() first");
        const Camera::Ptr cl = dataset_->GetCamera(left_cam_index_), cr = dataset_->GetCamera(right_cam_index_);
        // baseline = |pose_inv_.translation() of the two cameras| (:122-124); the kernel takes fx and it as floats (:120, :124)
        const SE3 il = cl->pose.inverse(), ir = cr->pose.inverse();
        const double baseline = std::sqrt((il.v[4] - ir.v[4]) * (il.v[4] - ir.v[4]) + (il.v[5] - ir.v[5]) * (il.v[5] - ir.v[5]) +
                                          (il.v[6] - ir.v[6]) * (il.v[6] - ir.v[6]));
        double cam[4];
        cl->k4(cam);
        const int B = 8;                           // keyframes per device call
        xyz_.clear(); bgr_.clear();
        std::vector<float> xyz;
        std::vector<int> pix;
        std::vector<uint8_t> bgr;                  // b, g, r of every point of the call, indexed like xyz
        const int ch = color_input_ ? 3 : 1;
        for (size_t k0 = 0; k0 < keyframes_.size(); k0 += (size_t)B) {
            const int nb = (int)std::min<size_t>((size_t)B, keyframes_.size() - k0);
            std::vector<Frame::Ptr> frames;
            for (int i = 0; i < nb; ++i) {
                Frame::Ptr f = dataset_->FrameById(keyframes_[k0 + (size_t)i].image_id);
                if (!f) throw SLAMException("DenseReconstruction: cannot read the images of keyframe " + std::to_string(keyframes_[k0 + (size_t)i].image_id));
                if (!kernels_) create(f->left_img_.cols, f->left_img_.rows);
                if (f->left_img_.cols != src_w_ || f->left_img_.rows != src_h_ || f->right_img_.cols != src_w_ || f->right_img_.rows != src_h_)
                    throw SLAMException("frame size changed");
                if (f->left_img_.channels != ch || f->right_img_.channels != ch) throw SLAMException("frame channels changed");
                frames.push_back(f);
            }
            std::vector<int> slots, planes, job_planes; std::vector<const void *> imgs; std::vector<int> strides;
            std::vector<svslam_dense_job> jobs((size_t)nb);
            const int cap = w_ * h_;
            for (int i = 0; i < nb; ++i) {
                slots.push_back(2 * i); slots.push_back(2 * i + 1);
                imgs.push_back(frames[(size_t)i]->left_img_.data.data()); imgs.push_back(frames[(size_t)i]->right_img_.data.data());
                strides.push_back(ch * src_w_); strides.push_back(ch * src_w_);
                planes.push_back(i); planes.push_back(-1); job_planes.push_back(i);          // the left image keeps its colours
                svslam_dense_job &j = jobs[(size_t)i];
                j.slot_left = 2 * i; j.slot_right = 2 * i + 1; j.pt_ofs = i * cap; j.n_points = 0;
                std::memcpy(j.T_cw, keyframes_[k0 + (size_t)i].T_cw.v, sizeof(j.T_cw));
            }
            xyz.resize(3 * (size_t)cap * (size_t)nb); pix.resize((size_t)cap * (size_t)nb); bgr.resize(3 * (size_t)cap * (size_t)nb);
            int rc;
            if (color_input_) {
                rc = kernels_->pyramid_bgr(2 * nb, slots.data(), planes.data(), imgs.data(), strides.data(), src_w_, src_h_, 0);
                if (rc == 0)
                    rc = kernels_->dense_cloud_bgr(nb, jobs.data(), cam, cl->pose.v, baseline, &params_, 1.0, cap, job_planes.data(), xyz.data(), pix.data(),
                                                   bgr.data(), nullptr);
            } else {
                rc = kernels_->pyramid_decimate(2 * nb, slots.data(), imgs.data(), strides.data(), src_w_, src_h_, 0);
                if (rc == 0) rc = kernels_->dense_cloud(nb, jobs.data(), cam, cl->pose.v, baseline, &params_, 1.0, cap, xyz.data(), pix.data(), nullptr);
                // grey input: b = g = r = the left pixel, dst(x, y) = src(2x, 2y) (src/dataset.cpp:162-165)
                for (int i = 0; rc == 0 && i < nb; ++i) {
                    const svslam_dense_job &j = jobs[(size_t)i];
                    const Image &src = frames[(size_t)i]->left_img_;
                    for (int q = 0; q < j.n_points; ++q) {
                        const size_t o = (size_t)j.pt_ofs + (size_t)q;
                        const int y = pix[o] / w_, x = pix[o] - y * w_;
                        bgr[3 * o] = bgr[3 * o + 1] = bgr[3 * o + 2] = src.data[(size_t)(2 * y) * (size_t)src_w_ + (size_t)(2 * x)];
                    }
                }
            }
            if (rc != 0) throw SLAMException(std::string("DenseReconstruction: ") + kernels_->last_error());
            // statistical_filter.filter(*tmp) of every keyframe cloud (:179-184): the call's keyframes are the segments of one batch
            std::vector<uint8_t> keep;
            if (cloud_filters_) {
                std::vector<float> packed;
                std::vector<int64_t> seg_ofs(1, 0);
                for (int i = 0; i < nb; ++i) {
                    const svslam_dense_job &j = jobs[(size_t)i];
                    packed.insert(packed.end(), xyz.begin() + 3 * (long)j.pt_ofs, xyz.begin() + 3 * ((long)j.pt_ofs + j.n_points));
                    seg_ofs.push_back(seg_ofs.back() + j.n_points);
                }
                keep.assign((size_t)seg_ofs.back() + 1, 1);
                std::vector<double> thr((size_t)nb);
                if (kernels_->cloud_sor(nb, seg_ofs.data(), packed.data(), 50, 1.0, keep.data(), thr.data()) != 0)
                    throw SLAMException(std::string("DenseReconstruction: ") + kernels_->last_error());
            }
            size_t kpos = 0;
            for (int i = 0; i < nb; ++i) {
                const svslam_dense_job &j = jobs[(size_t)i];
                for (int p = 0; p < j.n_points; ++p, ++kpos) {
                    if (cloud_filters_ && !keep[kpos]) continue;
                    const size_t o = (size_t)j.pt_ofs + (size_t)p;
                    xyz_.insert(xyz_.end(), xyz.begin() + 3 * (long)o, xyz.begin() + 3 * (long)o + 3);
                    bgr_.insert(bgr_.end(), bgr.begin() + 3 * (long)o, bgr.begin() + 3 * (long)o + 3);
                }
            }
        }
        if (cloud_filters_ && !bgr_.empty()) FilterMergedCloud();
        const std::string output_dir = config_.Str("output_dir", ".");
        map_file_ = output_dir + "/dense_map.pcd";
        if (!SavePCDFileBinary(map_file_)) throw SLAMException("DenseReconstruction: cannot write " + map_file_);
    }

    // :190-209 — the outlier removal once more on the merged cloud, then the 2 cm voxel grid with the points' colours (the grid
    // takes three bytes per point in any order and averages each: b, g, r go in and come out).  Grey input goes through as
    // r = g = b; the three sums of a voxel are the same sum, so the centroid's colour is grey again.
    void FilterMergedCloud()
    {
        const int64_t n = (int64_t)(bgr_.size() / 3);
        const int64_t seg_ofs[2] = { 0, n };
        std::vector<uint8_t> keep((size_t)n);
        double thr = 0;
        if (kernels_->cloud_sor(1, seg_ofs, xyz_.data(), 50, 1.0, keep.data(), &thr) != 0)
            throw SLAMException(std::string("DenseReconstruction: ") + kernels_->last_error());
        std::vector<float> fx;
        std::vector<uint8_t> frgb;
        for (size_t i = 0; i < (size_t)n; ++i) {
            if (!keep[i]) continue;
            fx.insert(fx.end(), xyz_.begin() + 3 * (long)i, xyz_.begin() + 3 * (long)i + 3);
            frgb.insert(frgb.end(), bgr_.begin() + 3 * (long)i, bgr_.begin() + 3 * (long)i + 3);
        }
        const int64_t nf = (int64_t)(frgb.size() / 3);
        std::vector<float> ox(3 * (size_t)nf + 3);
        std::vector<uint8_t> orgb(3 * (size_t)nf + 3);
        int64_t m = 0;
        int overflowed = 0;
        const double resolution = 0.02;
        if (kernels_->cloud_voxel_grid(nf, fx.data(), frgb.data(), resolution, ox.data(), orgb.data(), &m, &overflowed) != 0)
            throw SLAMException(std::string("DenseReconstruction: ") + kernels_->last_error());
        if (overflowed) std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
        xyz_.assign(ox.begin(), ox.begin() + 3 * (long)m);
        bgr_.assign(orgb.begin(), orgb.begin() + 3 * (long)m);
    }

    // pcl::io::savePCDFileBinary of a PointXYZRGB cloud: PCD v0.7, x y z rgb, the colour packed r << 16 | g << 8 | b into the
    // 4 bytes of the rgb field
    bool SavePCDFileBinary(const std::string &path) const
    {
        std::ofstream o(path, std::ios::binary);
        if (!o) return false;
        const size_t n = bgr_.size() / 3;
        o << "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F F\nCOUNT 1 1 1 1\nWIDTH " << n
          << "\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS " << n << "\nDATA binary\n";
        std::vector<char> rec(16 * n);
        for (size_t i = 0; i < n; ++i) {
            const uint32_t rgb = ((uint32_t)bgr_[3 * i + 2] << 16) | ((uint32_t)bgr_[3 * i + 1] << 8) | bgr_[3 * i];
            std::memcpy(&rec[16 * i], &xyz_[3 * i], 12);
            std::memcpy(&rec[16 * i + 12], &rgb, 4);
        }
        o.write(rec.data(), (std::streamsize)rec.size());
        return (bool)o;
    }

    const std::vector<DenseKeyframe> &Keyframes() const { return keyframes_; }
    size_t NumPoints() const { return bgr_.size() / 3; }
    const std::string &MapFile() const { return map_file_; }
    Dataset::Ptr dataset() { return dataset_; }
    K *kernels() { return kernels_.get(); }

private:
    void create(int w, int h)
    {
        src_w_ = w; src_h_ = h;
        w_ = (int)std::nearbyint(w * 0.5); h_ = (int)std::nearbyint(h * 0.5);
        svslam_limits lim;
        std::memset(&lim, 0, sizeof(lim));
        lim.device = (int)config_.Num("device", 0); lim.width = w_; lim.height = h_; lim.max_slots = 16; lim.max_jobs = 16;     // 8 keyframes per call: 16 images in one pyramid call
        lim.max_pts = 8; lim.max_corners = 8;
        kernels_.reset(new K(lim));
        if (color_input_ && kernels_->colour_reserve(8) != 0)                   // one plane per keyframe of a call
            throw SLAMException(std::string("DenseReconstruction: ") + kernels_->last_error());
    }
    std::string config_file_path_, slam_output_dir_, data_sequence_path_, map_file_;
    ConfigFile config_;
    int left_cam_index_ = 0, right_cam_index_ = 1, left_camera_index_in_slam_ = 0;
    int num_disparities_ = 128, blockSize_ = 15;   // include/StereoVisionSLAM/dense_reconstruction.h:56-57
    bool cloud_filters_ = false;                   // dense config `cloud_filters`: the PCL filters of :175-209
    bool color_input_ = false;                     // dense config `is_color_input`: colour images in, a coloured cloud out
    svslam_bm_params params_;
    std::vector<DenseKeyframe> keyframes_;
    Dataset::Ptr dataset_;
    std::unique_ptr<K> kernels_;
    int src_w_ = 0, src_h_ = 0, w_ = 0, h_ = 0;
    std::vector<float> xyz_;                      // the merged cloud: x y z per point ...
    std::vector<uint8_t> bgr_;                    // ... and its colour, b g r per point (grey input: three times the grey value)
};

} // namespace facade
} // namespace svs
