// Host check of smokephysai_amd/csrc/encoder_cells.h (tests/test_encoder_cells_host.py): the text the kernels compile.
//   encoder_cells <frames.f32> <B> <out.u8>
// frames: B frames of 256 x 256 floats.  Writes, per frame, tile row and tile column, two bytes (left cell live, right cell live) found
// by the pixel rule (enc_cell_window, words != 0 inside the image), checks that the scan's 4 x 4 flag-block rule (enc_cell_flag_col) gives
// the same bits, and prints the work list the cell words give (both-cells segment, then one-cell segment) as entries.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "encoder_cells.h"

using namespace smk;

int main(int argc, char **argv) {
    if (argc != 4) return 2;
    const int B = atoi(argv[2]), N = 256, TY = N / 8, TX = N / 16;
    std::vector<uint32_t> x((size_t)B * N * N);
    FILE *f = fopen(argv[1], "rb");
    if (!f || fread(x.data(), 4, x.size(), f) != x.size()) return 3;
    fclose(f);
    std::vector<uint8_t> bits((size_t)B * TY * TX * 2);
    long mismatches = 0;
    for (int b = 0; b < B; ++b) {
        const uint32_t *img = x.data() + (size_t)b * N * N;
        // the scan's flags: [row block + 1][column block + 1], one pad block all round
        std::vector<uint8_t> flag((size_t)(N / 4 + 2) * (N / 4 + 2), 0);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                if (img[i * N + j]) flag[(size_t)(i / 4 + 1) * (N / 4 + 2) + j / 4 + 1] = 1;
        for (int ty = 0; ty < TY; ++ty)
            for (int tx = 0; tx < TX; ++tx)
                for (int side = 0; side < 2; ++side) {
                    int rl, rh, cl, ch;
                    enc_cell_window(8 * ty, 16 * tx, side, rl, rh, cl, ch);
                    bool live = false;
                    for (int i = rl < 0 ? 0 : rl; i < (rh > N ? N : rh); ++i)
                        for (int j = cl < 0 ? 0 : cl; j < (ch > N ? N : ch); ++j) live |= img[i * N + j] != 0;
                    bool blocks = false;                      // the tile's flag rows start at block row 2 ty (pad included), 4 of them
                    for (int br = 0; br < 4; ++br)
                        for (int bc = 0; bc < ENC_CELL_FLAG_COLS; ++bc)
                            blocks |= flag[(size_t)(2 * ty + br) * (N / 4 + 2) + enc_cell_flag_col(tx, side) + bc] != 0;
                    mismatches += live != blocks;
                    bits[(((size_t)b * TY + ty) * TX + tx) * 2 + side] = live;
                }
    }
    f = fopen(argv[3], "wb");
    if (!f || fwrite(bits.data(), 1, bits.size(), f) != bits.size()) return 4;
    fclose(f);
    printf("BLOCK_RULE_MISMATCHES %ld\n", mismatches);

    // the work list from band words (a band = 4 tile rows x 16 tiles = 64 bits, bit = tile of the band)
    const int nbands = B * TY / 4;
    std::vector<unsigned long long> L(nbands, 0), R(nbands, 0);
    for (int t = 0; t < B * TY * TX; ++t) {
        if (bits[(size_t)t * 2]) L[t >> 6] |= 1ull << (t & 63);
        if (bits[(size_t)t * 2 + 1]) R[t >> 6] |= 1ull << (t & 63);
    }
    long tiles = 0, both = 0, one = 0;
    printf("ENTRIES");
    for (int seg = 0; seg < 2; ++seg)
        for (int j = 0; j < nbands; ++j) {
            const unsigned long long m = seg ? enc_cells_one(L[j], R[j]) : enc_cells_both(L[j], R[j]);
            for (int i = 0; i < 64; ++i)
                if ((m >> i) & 1) {
                    const int e = enc_entry(j * 64 + i, seg, (int)(~L[j] >> i) & 1);
                    if (enc_entry_tile(e) != j * 64 + i) return 5;
                    printf(" %d:%d", enc_entry_tile(e), enc_entry_cell(e));
                    (seg ? one : both) += 1;
                }
            if (seg == 0) tiles += __builtin_popcountll(enc_cells_tile(L[j], R[j]));
        }
    printf("\nTILES %ld BOTH %ld ONE %ld\n", tiles, both, one);

    // the one-cell body's pixels: conv1 covers exactly what conv2 reads, inside the tile's 10 x 18 a1 image
    for (int side = 0; side < 2; ++side) {
        bool c1[10 * ENC_CELL_AW] = {}, c2[10 * ENC_CELL_AW] = {};
        for (int pp = 0; pp < ENC_CELL_A1_PIX; ++pp) {
            int ar, ac;
            enc_cell_conv1_pixel(pp, side, ar, ac);
            if (ar < 0 || ar >= 10 || ac < 0 || ac >= ENC_CELL_AW || c1[ar * ENC_CELL_AW + ac]) return 6;
            c1[ar * ENC_CELL_AW + ac] = true;
        }
        bool out[8][8] = {};
        for (int m = 0; m < 4; ++m)
            for (int px = 0; px < 16; ++px) {
                const int centre = enc_cell_a1_pixel(m, px, 1, 1, side);       // tap (1, 1) is the output pixel itself, +1 halo
                const int orow = centre / ENC_CELL_AW - 1, ocol = centre % ENC_CELL_AW - 1 - 8 * side;
                if (orow < 0 || orow >= 8 || ocol < 0 || ocol >= 8 || out[orow][ocol]) return 7;
                out[orow][ocol] = true;
                for (int ki = 0; ki < 3; ++ki)
                    for (int kj = 0; kj < 3; ++kj) {
                        const int p = enc_cell_a1_pixel(m, px, ki, kj, side);
                        if (p < 0 || p >= 10 * ENC_CELL_AW) return 8;
                        c2[p] = true;
                    }
            }
        if (memcmp(c1, c2, sizeof c1) != 0) return 9;
    }
    printf("A1_PIXELS_OK\n");
    return 0;
}
