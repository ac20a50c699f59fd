// repair_device.hpp -- what ik_region.hip needs of ik_repair.hip: the refusals of a repair request and the launch of
// the repair pass over the region kernel's columns.
#pragma once

#include "constraint_device.hpp"

namespace optik {
namespace repairdev {

// The refusals of optik_hip_ik_region_repair's `repair`, before any device work: 0 or a fail() code.
int check_region_repair(const optik_hip_chain *ch, const optik_hip_region_repair *rep);

// region_repair_kernel on `stream` over the columns of one optik_hip_ik_region launch: x [n][cols], violation and key
// [cols] are the region kernel's and are updated in place; rep->d_repaired [T] (may be null) is zeroed and counted.
// keep: the region launch's ConstraintDev (its box is the keep box when keep_on).
int region_repair_launch(const optik_hip_chain *ch, const double *ee_offset7, const optik_hip_region_repair *rep,
                         const double *d_regions, const double *d_x0, int32_t T, unsigned long long R, size_t cols,
                         int mode, const condev::ProjectArgs &pr, const constraint::Box &keep_box, int keep_on,
                         double keep_tol, double *d_x, double *d_violation, double *d_key, hipStream_t stream);

}  // namespace repairdev
}  // namespace optik
