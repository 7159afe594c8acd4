// tpr_chain_args.hpp -- argument blocks of the rigid-body chain kernels (tpr_chain.hip.inc), shared with the C-ABI entries.
#pragma once
#include <cstdint>
namespace tpr {
constexpr int kChainRegMaxDof = 8;   // 1 .. 8 dof: compile-time dof, a point's state in registers; above: runtime dof, LDS
constexpr int kChainBlock = 64;      // threads per block of every chain kernel: one wave
// Doubles of LDS one thread keeps per link in the runtime-dof kernels: sine, cosine, and (force, moment) of each evaluation
// that the backward recursion reads -- 3 doubles for tau(q, 0, 0) (no moment without velocity and acceleration), 6 else.
constexpr int kChainSlotsSingle = 2 + 6, kChainSlotsFused = 2 + 3 + 6 + 6;
constexpr int kChainLdsBytes = 160 * 1024;

// tpr_chain with device pointers; the joint types by value as one bit per link (set = prismatic): wave-uniform by construction.
struct ChainModel {
    int d;
    uint32_t prismatic;
    const double *axis, *rot, *trans, *mass, *com, *inertia, *gravity, *tool;
};

struct ChainDynArgs {
    ChainModel M;
    int npoints;
    const double *q, *qd, *qdd;  // [npoints][d]
    double *tau;
};

struct ChainTermsArgs {
    ChainModel M;
    int npoints;
    const double *q, *qs, *qss;  // [npoints][d]
    double *w0, *wa, *wb;
};

struct ChainToolArgs {
    ChainModel M;
    int npoints, n1;      // B (N + 1); N + 1
    const double *q, *qs;  // [npoints][d]
    const double *S;       // [6][6] or null
    const double *limit;   // [B] or null
    double *vSv;           // [npoints] or null
    double *xbound;        // [npoints][2] or null
};

struct ChainAccelArgs {
    ChainModel M;
    int npoints;
    const double *q, *qd, *qdd;  // [npoints][d]
    double *acc;                 // [npoints][6]: linear, angular
};

struct ChainAccelTermsArgs {
    ChainModel M;
    int npoints;
    const double *q, *qs, *qss;  // [npoints][d]
    double *wa, *wb;             // [npoints][6]
};

// A rigid body fixed to the last link (tpr_payload), by value: the same for every lane.
struct ChainPayload {
    double mass, com[3], inertia[6], rot[9], origin[3];
};

struct ChainWrenchArgs {
    ChainModel M;
    ChainPayload P;
    int npoints;
    const double *q, *qd, *qdd;  // [npoints][d]
    double *wrench;              // [npoints][6]: force, moment about the contact frame's origin, contact-frame axes
};

struct ChainWrenchTermsArgs {
    ChainModel M;
    ChainPayload P;
    int npoints;
    const double *q, *qs, *qss;  // [npoints][d]
    double *w0, *wa, *wb;        // [npoints][6]
};
// Control points (tpr_chain_points), by value: points fixed in the frames of any links, the same set for every lane.
constexpr int kChainMaxPoints = 16;
constexpr int kChainPointsChunk = 3;  // links whose q, q', q'' the acceleration kernels stage in LDS at a time
struct ChainPoints {
    int32_t count, link[kChainMaxPoints];
    double offset[kChainMaxPoints][3];
};

struct ChainPointsSpeedArgs {
    ChainModel M;
    ChainPoints P;
    int npoints, n1, nlinks;  // B (N + 1); N + 1; the deepest link that carries a point, plus one
    const double *q, *qs;     // [npoints][d]
    const double *limit;      // [B][count] or null
    double *speed2;           // [npoints][count] or null
    double *xbound;           // [npoints][2] or null
};

// One block for both acceleration kernels: the single evaluation writes acc alone (wa is null).
struct ChainPointsAccelArgs {
    ChainModel M;
    ChainPoints P;
    int npoints, nlinks;         // nlinks as above
    const double *q, *v1, *v2;   // [npoints][d]: (q, qd, qdd), or (q, qs, qss)
    double *wa, *acc;            // [npoints][3 count]: acc(q, 0, v1) [terms only], acc(q, v1, v2)
};
}  // namespace tpr
