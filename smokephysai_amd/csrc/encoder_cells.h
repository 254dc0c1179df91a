#pragma once
// The cell rule of the encoder's tile skip at 256^2 (encoder.hip, "tile skip per pooled cell").  There PS = 8 and an 8 x 16 tile is two
// independent 8 x 8 pooled cells, each with its own 16 x 16 input window (cell + 4 pixels each way: conv1's 3 + conv2's 1).  A cell whose
// window is all-zero words equals the same cell of an all-zero frame, so a tile with one such cell runs a body of half the size.
// Plain C++ with no HIP type in it: a host program compiles exactly this text (tests/host/encoder_cells_main.cpp).
#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMK_ENC_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SMK_ENC_HD inline
#endif
namespace smk {

constexpr int ENC_CELL = 8;                 // a pooled cell at 256^2, and the tile's height
constexpr int ENC_CELL_HALO = 4;            // how far outside the cell its input window reaches
constexpr int ENC_CELL_A1 = ENC_CELL + 2;   // conv2's a1 window of a cell: 10 x 10 halo pixels
constexpr int ENC_CELL_A1_PIX = ENC_CELL_A1 * ENC_CELL_A1;
constexpr int ENC_CELL_AW = 18;             // a1 halo pixels per row of the tile's image (B3_AW)

// The pixel window of cell `side` (0 left, 1 right) of the tile whose first pixel is (r0, c0): rows [row_lo, row_hi) and columns
// [col_lo, col_hi), before clipping to the image.  The rows are the tile's own; the tile's window is the union of the two.
SMK_ENC_HD void enc_cell_window(int r0, int c0, int side, int &row_lo, int &row_hi, int &col_lo, int &col_hi) {
    row_lo = r0 - ENC_CELL_HALO;
    row_hi = r0 + ENC_CELL + ENC_CELL_HALO;
    col_lo = c0 + ENC_CELL * side - ENC_CELL_HALO;
    col_hi = c0 + ENC_CELL * side + ENC_CELL + ENC_CELL_HALO;
}
// The same window in the scan's 4 x 4 pixel blocks (window edges fall on multiples of 4): a flag row holds one pad block, then the
// frame's W / 4 blocks, then one pad block; tile column tx starts at block 4 tx of it, its window spans 6 blocks, a cell's
// ENC_CELL_FLAG_COLS of them from enc_cell_flag_col on.
constexpr int ENC_CELL_FLAG_COLS = 4;
SMK_ENC_HD int enc_cell_flag_col(int tx, int side) { return 4 * tx + 2 * side; }

// A band's two cell words (bit i = tile i of the band: left cell live, right cell live) -> the tile mask and the two segments of the
// work list: first every tile with both cells live, then every tile with exactly one, each in ascending order.
SMK_ENC_HD unsigned long long enc_cells_tile(unsigned long long l, unsigned long long r) { return l | r; }
SMK_ENC_HD unsigned long long enc_cells_both(unsigned long long l, unsigned long long r) { return l & r; }
SMK_ENC_HD unsigned long long enc_cells_one(unsigned long long l, unsigned long long r) { return l ^ r; }

// A work-list entry: the tile, and above ENC_ENTRY_SHIFT what to run of it: 0 both cells, 2 the left cell only, 3 the right cell only.
constexpr int ENC_ENTRY_SHIFT = 29, ENC_ENTRY_TILE = (1 << ENC_ENTRY_SHIFT) - 1;
SMK_ENC_HD int enc_entry(int tile, bool one_cell, int side) { return tile | (one_cell ? (2 | side) << ENC_ENTRY_SHIFT : 0); }
SMK_ENC_HD int enc_entry_tile(int entry) { return entry & ENC_ENTRY_TILE; }
SMK_ENC_HD int enc_entry_cell(int entry) { return entry >> ENC_ENTRY_SHIFT; }

// The one-cell body.  conv1 covers the 10 x 10 a1 pixels the cell's conv2 reads: pixel pp (0 .. 99) -> halo row and column of the tile's
// a1 image (the image offsets are those of a whole tile).
SMK_ENC_HD void enc_cell_conv1_pixel(int pp, int side, int &ar, int &ac) {
    ar = pp / ENC_CELL_A1;
    ac = ENC_CELL * side + pp - ar * ENC_CELL_A1;
}
// conv2 has 4 M blocks of 16 pixels: block m = cell rows 2m, 2m + 1 x the cell's 8 columns, operand lane px = row px >> 3, column px & 7.
// The a1 halo pixel lane px reads for tap (ki, kj):
SMK_ENC_HD int enc_cell_a1_pixel(int m, int px, int ki, int kj, int side) {
    return (2 * m + (px >> 3) + ki) * ENC_CELL_AW + ENC_CELL * side + (px & 7) + kj;
}

}  // namespace smk
