// fdw_internal.h -- what the translation units of libfdwave.so share beyond the public header (include/fdwave.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "fdwave.h"

// sets fdw_last_error() of the calling thread and returns `code`
int fdw_fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// return FDW_EHIP (with the failing call in fdw_last_error()) / any other error code from the enclosing function
#define HIP_TRY(call)                                                                                            \
    do {                                                                                                         \
        hipError_t e_ = (call);                                                                                  \
        if (e_ != hipSuccess) return fdw_fail(FDW_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define FDW_TRY(call)              \
    do {                           \
        int rc_ = (call);          \
        if (rc_ != FDW_OK) return rc_; \
    } while (0)

// the two of four rotating buffers that hold neither a nor b, in index order
inline void spare_pair(int a, int b, int* o1, int* o2)
{
    int n = 0;
    for (int i = 0; i < 4; i++)
        if (i != a && i != b) (n++ == 0 ? *o1 : *o2) = i;
}

// every receiver row (interior rows nxb .. nxb+nx-1 of the global grid, R:126-129) lies below xlim, i.e. is time-stepped: the wave-pipeline
// passes of the backward loop and the batched shots have no static-row epilogue for the others
int fdw_receivers_stepped(const fdw_ctx* c);

// The launches of the slab driver's recording forward loop (fdw_api.cpp): fdw_dev_step (mode FWD) and fdw_dev_step4 on row ranges of a slab
// that also write their trace rows -- d_rec_row: this step's samples [nx], d_rec: the four rows of the pass, indexed by GLOBAL receiver
// (rec[g - nxb] for global row g); NULL: the plain launch --, the samples of receiver rows the loop never time-steps for a whole call
// (from the fields before the first swap), and fdw_record_shot's check of the receiver depth and the dialect.
int fdw_dev_step_rec(fdw_ctx* c, const float* d_p, float* d_pp, const float* d_v2, int r0, int r1, int pp_twice, const float* d_srce_it, int sx, int sz,
                     float* d_rec_row, int gz, hipStream_t s);
int fdw_dev_step4_rec(fdw_ctx* c, const float* d_p, const float* d_pp, const float* d_v2, float* d_out1, float* d_out2, int pp_twice, const float* d_srce_it,
                      int sx, int sz, int r0, int r1, int r0b, int r1b, int xchunk, float* d_rec, int gz, hipStream_t s);
int fdw_dev_record_static(fdw_ctx* c, const float* d_p, const float* d_pp, int gz, float* d_rec, int it0, int nsteps, hipStream_t s);
int fdw_check_record_depth(const fdw_ctx* c, int gz);

constexpr int FDW_COMM_MAX_FIELDS = 8;

// Halo exchange of `nfields` fields with the two neighbouring ranks, enqueued on `stream` (fdw_comm.cpp)
int fdw_comm_exchange(fdw_comm* c, int nfields, float* const* fields, size_t send_lo, size_t recv_lo, size_t send_hi, size_t recv_hi,
                      size_t count, hipStream_t stream);

// A roctx range for the lifetime of the object (fdw_trace.cpp): FDW_RANGE("forward loop"); no-op unless a marker library is in the process
struct fdw_range {
    explicit fdw_range(const char* name);
    ~fdw_range();
    fdw_range(const fdw_range&) = delete;
    fdw_range& operator=(const fdw_range&) = delete;
    bool active;
};
#define FDW_RANGE_CAT2(a, b) a##b
#define FDW_RANGE_CAT(a, b) FDW_RANGE_CAT2(a, b)
#define FDW_RANGE(name) fdw_range FDW_RANGE_CAT(fdw_range_, __LINE__)(name)
