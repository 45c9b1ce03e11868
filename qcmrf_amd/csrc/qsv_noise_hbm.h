// qsv_noise_hbm.h -- noisy shots whose trajectories live in device memory (qsv_noisy_sample_hbm): the launcher.  Shared by
// qsv_noise_hbm.hip (kernel) and qsv.hip (entry point in qsv_exec.inc).  The record (NzOp), the Philox draws and NzMeas are
// those of qsv_noise.h.
#pragma once
#include "qsv_noise.h"

#define QSV_NZ_HBM_MAXW 24        // 2^24 complex128 = 256 MiB per trajectory; index arithmetic stays in 32 bits
#define QSV_NZ_HBM_TPB 256

struct NzHbmLaunch : NzCall {
  unsigned grid;            // workgroups = slots; the caller sized `slots` for it
  char* d_slots;            // grid x (16 << W) bytes: workgroup b owns [b (16 << W), (b + 1) (16 << W))
};

// workgroups of the trajectory kernel the chip holds at once (occupancy API x n_cu), at least 1
hipError_t qsv_noise_hbm_resident(int n_cu, uint64_t* workgroups);
// launches the trajectory kernel on l.stream (asynchronous)
hipError_t qsv_noise_hbm_launch(const NzHbmLaunch& l);
// the same for a stream that holds an NZ_MEASURE op (qsv_noise_measure.hip); qsv_noise_hbm_launch comes here by itself
hipError_t qsv_noise_hbm_launch_measure(const NzHbmLaunch& l);
// the accept-aware kernel (qsv_noise_accept.hip), for any stream, after the checks of qsv_noise_hbm_launch
hipError_t qsv_noise_hbm_launch_accept(const NzHbmLaunch& l, const NzAccept& a);
// the two launches above for a stream that holds an NZ_KRAUS2 op (qsv_noise_kraus2.hip), after their checks; they come here by
// themselves
hipError_t qsv_noise_hbm_launch_kraus2(const NzHbmLaunch& l);
hipError_t qsv_noise_hbm_launch_accept_kraus2(const NzHbmLaunch& l, const NzAccept& a);
// the same two for a stream with l.dynamic (qsv_noise_dynamic.hip), after their checks and before l.kraus2 is looked at
hipError_t qsv_noise_hbm_launch_dynamic(const NzHbmLaunch& l);
hipError_t qsv_noise_hbm_launch_accept_dynamic(const NzHbmLaunch& l, const NzAccept& a);
