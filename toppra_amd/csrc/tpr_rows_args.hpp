// tpr_rows_args.hpp -- argument block of the row-assembly kernels (tpr_rows.hip.inc), shared with the C-ABI entries.
#pragma once
#include <cstdint>
namespace tpr {
constexpr int kRowsMaxBlocks = 8;  // second-order constraints in one list (tpr_second_order_rows_batch)

// One second-order constraint: tpr_second_order_block with device pointers and its place in a stage's rows.
struct RowsBlock {
    int p, m;      // width of w; rows of F per gridpoint (2 p for the signed identity)
    int flags;     // TPR_SO_*
    int col0;      // first column of the block in a stage's nC rows
    int lds0;      // offset (doubles per staged gridpoint) of the block's a | b | c in a gridpoint's LDS record
    const double *w0, *wa, *wb;  // [B][N+1][p]
    const double *F, *g, *friction;
};

struct RowsArgs {
    int B, d, nseg, N, flags;  // as tpr_problem
    const double *coef, *breaks, *grid, *vlim, *alim;
    int nC;       // rows per stage, the two reserved ones included
    int nblocks;
    int wsum;     // sum of 3 p over the blocks: doubles per staged gridpoint
    RowsBlock blk[kRowsMaxBlocks];
};

// The same rows for a path given as samples at the gridpoints (tpr_sampled_rows_batch): coef / breaks stay null, nseg 0.
struct SampledRowsArgs : RowsArgs {
    const double *qs, *qss;  // [B][N+1][d]
    double *xbound;          // [B][N+1][2] or null: the velocity constraint's own x bound
};

struct PathEvalArgs {
    int B, d, nseg, N, flags;
    const double *coef, *breaks, *grid;
    double *q, *qs, *qss;  // [B][N+1][d], any may be nullptr
};
}  // namespace tpr
