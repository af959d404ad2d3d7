// The launchers of k_chol.hip that the distributed driver (dist_solve.hip) calls: host prototypes only — a kernel
// is launched from the file that defines it.  All enqueue on the stream they are given.
#pragma once
#include "engine.h"

namespace bae {

// the serial chain of one outer panel [J, Jend); rl / rl_n / rl_square: a row list instead of every row below
void launch_panel_chain(const CholSwitches& sw, hipStream_t s, double* dA, uint32_t ld, uint32_t nblk, uint32_t J,
                        uint32_t Jend, double* dsgn, double* opbuf, int* colneg, int* flags, const uint8_t* nz,
                        const uint32_t* rl = nullptr, uint32_t rl_n = 0, bool rl_square = false, bool sq = false);
// k_step_update<true>: tile columns [c0, c0 + grid.y) of grid.x row tiles (rl, or every row from c0) updated with
// the tile columns [kb0, kb1); workgroup (0, 0) factorises tile (c0, c0)
void launch_step_update(hipStream_t s, dim3 grid, double* dA, uint32_t ld, uint32_t nblk, uint32_t c0, uint32_t kb0,
                        uint32_t kb1, double* dsgn, double* opbuf, int* colneg, int* flags, const uint8_t* nz,
                        const uint32_t* rl);
// the rectangle below the tile columns [c0, c0 + ncols) in 128x128 blocks (rect128_shape said use128)
void launch_rect128(const CholSwitches& sw, const Rect128Shape& r, hipStream_t s, double* dA, uint32_t ld, uint32_t nblk,
                    uint32_t c0, uint32_t ncols, uint32_t kb0, uint32_t kb1, const double* dsgn, const int* colneg,
                    const uint8_t* nz, const OwnMap& own);
// bulk trailing update of the tile rows / columns >= a_end with the tile columns [J, Jend) (bulk_shape); blocks /
// nblocks: the launch's slice of the list of non-empty blocks (bulk_lists.h), sentinels included
void launch_bulk_update(const CholSwitches& sw, Engine* e, hipStream_t s, double* dA, uint32_t ld, uint32_t nblk,
                        uint32_t a_end, uint32_t J, uint32_t Jend, const double* dsgn, const int* colneg,
                        const uint8_t* nz, bool full, const OwnMap& own, const uint2* pairs = nullptr,
                        uint32_t npairs = 0, const uint2* blocks = nullptr, uint32_t nblocks = 0);
// L_JJ^-T of every diagonal tile from its factor packet
void launch_linvT(hipStream_t s, uint32_t nblk, const double* opbuf, const double* dsgn, double* linvT);
// the backward substitution over the block rows [lo, hi), last first
void launch_backward(hipStream_t s, double* dA, uint32_t ld, uint32_t nblk, const double* linvT, double* dx,
                     const uint8_t* nz, uint32_t lo = 0, uint32_t hi = 0xffffffffu);
// status block of a factorisation: cleared, with the pivot floors if the options ask for them
int setup_status_block(Engine* e, const double* dA, uint32_t ld, hipStream_t s0);

}  // namespace bae
