// stac_shapes.hpp -- the kernel instantiations that ship, and the one lookup the host plans its launches with.
//
// launch_q_phase (stac_kernels.hip) and launch_q_phase_lm (stac_lm.hip) expand these tables into their templates; the host
// (stac_q.hip, plan_q / plan_q_lm) asks q_shape which row a launch gets.
#pragma once

// ---- the instantiations that ship -------------------------------------------------------------------------------------------
// (lanes per chain G, solver registers per lane NQR: nq <= G * NQR, register cap WPE).  Every shape here passes the resource
// gate of tests/test_isa_hazards.py (scratch <= 64 B per lane, <= 40 scalars spilled into vector lanes; table:
// profiles/r04/resource_usage.txt).  What does not is not built: the 128-VGPR variants of the 8- and 16-lane kernels (74 to 750
// spilled vector registers) and of the 32- / 64-lane kernels with four or more solver registers per lane (17 to 80), 32 solver registers per lane at 4 or 8 lanes and the 4-lane kernels altogether (160 B to 1.3 KB of
// scratch; never chosen automatically, slower than 16 lanes at every batch size) -- a request for them runs on the next wider
// group, results are the same bit for bit.  Latency kernels stop at 10 solver registers per lane at 8 lanes and 8 at 16 or 32
// (round 3: the wider ones, 300+ B of scratch, read spill slots before writing them); wider models take more lanes per role.
#ifdef STAC_INST_SUBSET  // developer builds (experiments): only the shapes of the default bench and of its 250-frame-clip leg
#define STAC_Q_SHAPES(X) X(16, 5, 2) X(16, 5, 3)
#define STAC_Q_LEAN_SHAPES(X) X(16, 5, 3)
#define STAC_Q_SPEC_LEAN_SHAPES(X) X(16, 5, 4) X(16, 5, 8) X(32, 3, 8)
#define STAC_Q_SPEC_SHAPES(X) X(16, 5, 4) X(32, 3, 8)
#else
// lean kernels (SPECP bit 0): the shapes that rodent-sized models run in -- large batches, the straggler hand-off, few long clips
// (the first shape of a width that holds nq is taken: narrower ones first.  Three solver registers per lane at 16 lanes, two at 32: models of
//  up to 48 / 64 coordinates -- the fruit fly's 43 --, whose nq-sums and staging then run over three registers instead of five)
#define STAC_Q_LEAN_SHAPES(X) X(16, 3, 3) X(16, 5, 2) X(16, 5, 3) X(32, 3, 2) X(32, 8, 2)
#define STAC_Q_SPEC_LEAN_SHAPES(X) X(16, 3, 4) X(16, 5, 4) X(16, 5, 8) X(32, 2, 8) X(32, 3, 8) X(32, 8, 8)
#define STAC_Q_SHAPES(X)                                                        \
    X(8, 10, 2) X(8, 16, 2)                                                      \
    X(16, 5, 2) X(16, 5, 3) X(16, 8, 2) X(16, 8, 3) X(16, 16, 2)                 \
    X(32, 3, 2) X(32, 3, 4) X(32, 4, 2) X(32, 8, 2)                              \
    X(64, 2, 2) X(64, 2, 4) X(64, 4, 2)
// (G lanes per role, NQR, roles per chain)
#define STAC_Q_SPEC_SHAPES(X)                                                   \
    X(8, 10, 4) X(8, 10, 8) X(16, 5, 4) X(16, 8, 4) X(32, 3, 8) X(32, 8, 8) X(64, 2, 8) X(64, 4, 8)
#endif
// LM kernel (G, NQR, waves per SIMD of its register cap): the 64-lane instantiations fit 168 VGPRs (3 waves per SIMD), the
// narrower ones need 2 per SIMD
#define STAC_LM_SHAPES(X) X(16, 5, 2) X(16, 8, 2) X(16, 16, 2) X(32, 3, 2) X(32, 8, 2) X(64, 2, 3) X(64, 4, 2)

namespace stac {

// One instantiation: q_phase_kernel<G, NQR, WPE, SPECP> (SPECP bit 0 = the lean kernel, SPECP & ~1 = evaluation roles of the
// latency mode, 0 = throughput), or q_phase_lm_kernel<G, NQR, WPE> (WPE = waves per SIMD, SPECP = 0)
struct QInst { int G, nqr, wpe, specp; };

enum QKind { kThr, kThrLean, kLat, kLatLean, kLm };  // the table of each kind of kernel
struct QShapeRow { int G, nqr, third; };  // third: register cap (throughput), roles per chain (latency), waves per SIMD (LM)
#define STAC_ROW(GG, RR, TT) QShapeRow{GG, RR, TT},
constexpr QShapeRow kThrRows[] = {STAC_Q_SHAPES(STAC_ROW)}, kThrLeanRows[] = {STAC_Q_LEAN_SHAPES(STAC_ROW)},
                    kLatRows[] = {STAC_Q_SPEC_SHAPES(STAC_ROW)}, kLatLeanRows[] = {STAC_Q_SPEC_LEAN_SHAPES(STAC_ROW)},
                    kLmRows[] = {STAC_LM_SHAPES(STAC_ROW)};
#undef STAC_ROW

template <int N>
constexpr QShapeRow first_row(const QShapeRow (&rows)[N], int G, int nq, int third) {
    for (const QShapeRow &r : rows)
        if (r.G == G && nq <= r.G * r.nqr && (third == 0 || r.third == third)) return r;
    return QShapeRow{G, 0, third};
}
// The first row of `kind`'s table with G lanes that holds nq coordinates and has this third column (0: any); nqr == 0 if none
constexpr QShapeRow q_shape(QKind kind, int G, int nq, int third = 0) {
    switch (kind) {
        case kThr: return first_row(kThrRows, G, nq, third);
        case kThrLean: return first_row(kThrLeanRows, G, nq, third);
        case kLat: return first_row(kLatRows, G, nq, third);
        case kLatLean: return first_row(kLatLeanRows, G, nq, third);
        default: return first_row(kLmRows, G, nq, third);
    }
}

}  // namespace stac
