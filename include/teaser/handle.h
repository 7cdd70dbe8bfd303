// teaser/handle.h -- the library handles that the classes of this directory create on first use and own.
#pragma once

#include <stdexcept>
#include <string>

#include "teaser_hip.h"

namespace teaser {
namespace detail {

// Owns one handle of type H: nullptr until the derived holder's create(), destroyed with the holder.  Converts to
// H* so that it stands where the C functions take the handle.
template <class H, int32_t (*Destroy)(H*)>
class LazyHandle {
 public:
  LazyHandle() = default;
  LazyHandle(const LazyHandle&) = delete;
  LazyHandle& operator=(const LazyHandle&) = delete;
  ~LazyHandle() {
    if (h_) Destroy(h_);
  }
  operator H*() const { return h_; }

 protected:
  // rc: what teaser_hip_<kind>_create returned when it filled h_; `who` is the class the exception names.
  void created(const char* who, const char* kind, int32_t rc) {
    if (rc == TEASER_HIP_OK) return;
    h_ = nullptr;
    throw std::runtime_error(std::string(who) + ": teaser_hip_" + kind + "_create failed (status " +
                             std::to_string(rc) + "; 3 = no HIP device)");
  }
  H* h_ = nullptr;
};

struct LazySolver : LazyHandle<teaser_hip_solver, teaser_hip_solver_destroy> {
  // Creates the solver from `params` (nullptr: the defaults) on the current device unless it exists already;
  // returns whether this call created it.  Throws std::runtime_error when it cannot (no MI355X: no CPU path).
  bool create(const char* who, const teaser_params_c* params = nullptr) {
    if (h_) return false;
    created(who, "solver", teaser_hip_solver_create(params, /*device=*/-1, &h_));
    return true;
  }
};

struct LazyFeatures : LazyHandle<teaser_hip_features, teaser_hip_features_destroy> {
  void create(const char* who) {
    if (!h_) created(who, "features", teaser_hip_features_create(/*device=*/-1, &h_));
  }
};

struct LazyPoseGraph : LazyHandle<teaser_hip_posegraph, teaser_hip_posegraph_destroy> {
  void create(const char* who) {
    if (!h_) created(who, "posegraph", teaser_hip_posegraph_create(/*device=*/-1, &h_));
  }
};

struct LazyRansac : LazyHandle<teaser_hip_ransac, teaser_hip_ransac_destroy> {
  void create(const char* who) {
    if (!h_) created(who, "ransac", teaser_hip_ransac_create(/*device=*/-1, &h_));
  }
};

struct LazyFgr : LazyHandle<teaser_hip_fgr, teaser_hip_fgr_destroy> {
  void create(const char* who) {
    if (!h_) created(who, "fgr", teaser_hip_fgr_create(/*device=*/-1, &h_));
  }
};

struct LazyPlane : LazyHandle<teaser_hip_plane, teaser_hip_plane_destroy> {
  void create(const char* who) {
    if (!h_) created(who, "plane", teaser_hip_plane_create(/*device=*/-1, &h_));
  }
};

// A TSDF handle IS its volume, so it is created from the volume's record; the status is returned (the class that owns
// the holder throws its own error with it) and h_ stays nullptr unless it is TEASER_HIP_OK.
struct LazyTsdf : LazyHandle<teaser_hip_tsdf, teaser_hip_tsdf_destroy> {
  int32_t create(const teaser_tsdf_volume_c& volume, int32_t device = -1) {
    if (h_) return TEASER_HIP_OK;
    const int32_t rc = teaser_hip_tsdf_create(&volume, device, &h_);
    if (rc != TEASER_HIP_OK) h_ = nullptr;
    return rc;
  }
};

// Likewise for the scalable TSDF volume.
struct LazyStsdf : LazyHandle<teaser_hip_stsdf, teaser_hip_stsdf_destroy> {
  int32_t create(const teaser_stsdf_volume_c& volume, int32_t device = -1) {
    if (h_) return TEASER_HIP_OK;
    const int32_t rc = teaser_hip_stsdf_create(&volume, device, &h_);
    if (rc != TEASER_HIP_OK) h_ = nullptr;
    return rc;
  }
};

}  // namespace detail
}  // namespace teaser
