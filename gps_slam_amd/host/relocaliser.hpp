// FernRelocLib::Relocaliser (InfiniTAM/FernRelocLib/Relocaliser.h) over the device relocaliser of the C ABI (gps_reloc_*,
// csrc/reloc_fern.hip).  Where the reference's ProcessFrame downloads the depth image and answers on the CPU, this one enqueues
// four launches on the caller's stream and returns; ReadResult() fetches the answer (and synchronises the stream), so a caller
// that only needs the answer on a failed frame reads nothing back on a good one.
//   ProcessFrame(depth, M, invM, sceneId, k, harvest, stream)   Relocaliser.h:48-84, enqueued
//   ReadResult(stream)                                          hasAddedKeyframe / nearestNeighbours / distances of that frame
//   RetrievePose(id, stream)                                    PoseDatabase::retrievePose
//   SaveToDirectory / LoadFromDirectory                         the reference's config.txt, ferns.txt, frames.txt, poses.txt
//                                                               (relocaliser.cpp; host-synchronous)
#pragma once
#include <array>
#include <stdexcept>
#include <string>
#include <vector>

#include "gps_slam_hip.h"

namespace FernRelocLib {

struct PoseInScene { float M[16], invM[16]; int sceneIdx; };   // PoseDatabase.h:14-20 (pose in ORUtils layout)

namespace detail {
// the four text files as host data (relocaliser.cpp); poses: M then invM per entry, params: the six SE3 parameters of poses.txt
struct DatabaseFiles {
    int numFerns = 0, numDecisions = 0, totalEntries = 0;
    float harvestingThreshold = 0.f;
    std::vector<int32_t> xy, sceneIds;
    std::vector<float> thresholds, poses;
    std::vector<uint8_t> codes;
    std::vector<std::array<float, 6>> params;
};
DatabaseFiles readDatabase(const std::string& dir, int numFerns, int numDecisions, float harvestingThreshold);
void writeDatabase(const DatabaseFiles& db, const std::string& dir);
void poseFromParams(const float* params6, float* M, float* invM);
void paramsFromPose(const float* M, float* params6);
void saveToDirectory(gps_reloc_state* state, float harvestingThreshold, const std::vector<std::array<float, 6>>& knownParams,
                     const std::string& dir, gps_stream stream);
void loadFromDirectory(gps_reloc_state* state, float harvestingThreshold, std::vector<std::array<float, 6>>& knownParams,
                       const std::string& dir, gps_stream stream);
}  // namespace detail

template <typename ElementType>
class Relocaliser {
    static_assert(sizeof(ElementType) == sizeof(float), "the device relocaliser encodes float depth images");

public:
    // Relocaliser.h:27 + the database's capacity in keyframes and the fern table's seed (the reference draws its table from rand())
    Relocaliser(int width, int height, float rangeMin, float rangeMax, float harvestingThreshold, int numFerns, int numDecisionsPerFern,
                int capacity = 4096, uint64_t seed = 0) : threshold_(harvestingThreshold) {
        check(gps_reloc_create(&state_, width, height, numFerns, numDecisionsPerFern, rangeMin, rangeMax, harvestingThreshold, capacity,
                               seed), "gps_reloc_create");
    }
    ~Relocaliser() { if (state_) (void)gps_reloc_destroy(state_); }
    Relocaliser(const Relocaliser&) = delete;
    Relocaliser& operator=(const Relocaliser&) = delete;

    void ProcessFrame(const ElementType* depth_device, const float* M, const float* invM, int sceneId, int k, bool harvestKeyframes,
                      gps_stream stream) {
        check(gps_reloc_process_frame(state_, reinterpret_cast<const float*>(depth_device), M, invM, sceneId, k, harvestKeyframes ? 1 : 0,
                                      stream), "gps_reloc_process_frame");
    }
    gps_reloc_result ReadResult(gps_stream stream) {
        gps_reloc_result r;
        check(gps_reloc_read_result(state_, &r, stream), "gps_reloc_read_result");
        return r;
    }
    PoseInScene RetrievePose(int id, gps_stream stream) {
        PoseInScene p;
        int32_t scene = 0;
        check(gps_reloc_retrieve_pose(state_, id, p.M, p.invM, &scene, stream), "gps_reloc_retrieve_pose");
        p.sceneIdx = scene;
        return p;
    }
    int numEntries(gps_stream stream) {
        int32_t n = 0;
        check(gps_reloc_export(state_, 0, nullptr, nullptr, nullptr, &n, nullptr, stream), "gps_reloc_export");
        return n;
    }
    gps_reloc_state* state() { return state_; }
    // Relocaliser.h:91-118; the directory name ends in '/'.  Loading replaces the fern table and the database.
    void SaveToDirectory(const std::string& outputDirectory, gps_stream stream = nullptr) {
        detail::saveToDirectory(state_, threshold_, loaded_params_, outputDirectory, stream);
    }
    void LoadFromDirectory(const std::string& inputDirectory, gps_stream stream = nullptr) {
        detail::loadFromDirectory(state_, threshold_, loaded_params_, inputDirectory, stream);
    }

private:
    static void check(int status, const char* what) {
        if (status != GPS_OK) throw std::runtime_error(std::string(what) + " failed (" + std::to_string(status) + ")");
    }
    gps_reloc_state* state_ = nullptr;
    float threshold_;
    std::vector<std::array<float, 6>> loaded_params_;   // of the entries a file brought: poses.txt gets them back unchanged
};

}  // namespace FernRelocLib
