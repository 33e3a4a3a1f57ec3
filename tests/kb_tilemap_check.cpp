// kb_tilemap_check.cpp - the step round's "block index -> (list, tile, count)" map (csrc/fsq_kb_tilemap.h) checked on the CPU.
// For every combination of the six list counts drawn from {0, 1, 63, 64, 65, 130}: the blocks 0 .. sum(ceil(n / 64)) + 5 must
// cover every position of every list exactly once, the lists must come in the launch order C3, B10, C1, B3, B1, B0 with the
// tiles of a list in ascending order, every block past the last tile must map to "return", and the grid the host launches for
// that many fits must hold all the tiles.  Also: the history -> list rule, and that the two lists of an array never share a
// position while their counts add up to at most the capacity.
// Built by tests/test_kb_tilemap_host.py as a plain host program with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../fluorosequencingimageanalysis_amd/csrc/fsq_kb_tilemap.h"

static long long g_bad = 0;
#define CHECK(cond) do { if (!(cond)) { if (g_bad++ < 10) fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

int main()
{
    const int vals[6] = {0, 1, 63, 64, 65, 130};
    const int order[KB_LISTS] = {KB_C3, KB_B10, KB_C1, KB_B3, KB_B1, KB_B0};
    long long combos = 0, blocks = 0, positions = 0;
    for (int k = 0; k < KB_LISTS; k++) CHECK(kb_launch_order(k) == order[k]);
    int code[KB_LISTS];
    for (code[0] = 0; code[0] < 6; code[0]++) for (code[1] = 0; code[1] < 6; code[1]++) for (code[2] = 0; code[2] < 6; code[2]++)
    for (code[3] = 0; code[3] < 6; code[3]++) for (code[4] = 0; code[4] < 6; code[4]++) for (code[5] = 0; code[5] < 6; code[5]++) {
        int n[KB_LISTS];
        long long tiles = 0, alive = 0;
        for (int l = 0; l < KB_LISTS; l++) { n[l] = vals[code[l]]; tiles += (n[l] + 63) / 64; alive += n[l]; }
        std::vector<std::vector<int>> seen(KB_LISTS);
        for (int l = 0; l < KB_LISTS; l++) seen[l].assign((size_t)n[l], 0);
        int rank_prev = -1, tile_prev = -1;          // position of the previous block's list in the launch order, its tile
        for (long long b = 0; b <= tiles + 5; b++) {
            const KbTile t = kb_tile_of_block(b, n);
            blocks++;
            if (b >= tiles) { CHECK(t.list < 0); continue; }
            CHECK(t.list >= 0 && t.list < KB_LISTS);
            if (t.list < 0 || t.list >= KB_LISTS) continue;
            CHECK(t.count == n[t.list]);
            CHECK(t.tile >= 0 && (long long)t.tile * KB_TILE < t.count);
            int rank = -1;
            for (int k = 0; k < KB_LISTS; k++) if (order[k] == t.list) rank = k;
            CHECK(rank > rank_prev || (rank == rank_prev && t.tile == tile_prev + 1));
            if (rank > rank_prev) CHECK(t.tile == 0);
            rank_prev = rank; tile_prev = t.tile;
            for (int lane = 0; lane < KB_TILE; lane++) {
                const long long p = (long long)t.tile * KB_TILE + lane;
                if (p < t.count) { seen[t.list][(size_t)p]++; positions++; }       // (what kB_step's `live` admits)
            }
        }
        for (int l = 0; l < KB_LISTS; l++)
            for (int p = 0; p < n[l]; p++) CHECK(seen[l][(size_t)p] == 1);
        CHECK(kb_tile_of_block(-1, n).list < 0);
        CHECK(kb_grid_for(alive) >= tiles);
        combos++;
    }
    // the host's grid bound for any split of `alive` fits: six partial tiles at the worst
    for (long long alive = 0; alive < 1000; alive++) CHECK(kb_grid_for(alive) == (alive + 63) / 64 + 6);
    {
        const int n[KB_LISTS] = {1, 1, 1, 1, 1, 1};
        CHECK(kb_grid_for(6) == 7 && kb_tile_of_block(5, n).list == KB_B0 && kb_tile_of_block(6, n).list < 0);
        const int big[KB_LISTS] = {2147483647, 0, 0, 0, 0, 0};          // no overflow in the tile count
        CHECK(kb_tile_of_block(33554431, big).list == KB_B0 && kb_tile_of_block(33554431, big).tile == 33554431);
        CHECK(kb_tile_of_block(33554432, big).list < 0);
    }
    // history -> list
    for (int h = -3; h <= 40; h++) {
        const int l = kb_list_of_history(h);
        CHECK(l == (h <= 0 ? KB_B0 : h == 1 ? KB_B1 : h <= 4 ? KB_B3 : KB_B10));
    }
    // two lists per array, growing towards each other: no shared position while the counts fit the capacity
    CHECK(kb_list_array(KB_B0) == 0 && kb_list_array(KB_B1) == 0 && kb_list_array(KB_B3) == 1 && kb_list_array(KB_B10) == 1);
    for (int l = 0; l < KB_LISTS; l += 2) {
        CHECK(!kb_list_down(l) && kb_list_down(l + 1));
        const long long cap = 256;
        for (long long up = 0; up <= cap; up += 37) {
            const long long down = cap - up;
            std::vector<int> hit((size_t)cap, 0);
            for (long long p = 0; p < up; p++) hit[(size_t)kb_list_pos(l, p, cap)]++;
            for (long long p = 0; p < down; p++) hit[(size_t)kb_list_pos(l + 1, p, cap)]++;
            for (long long p = 0; p < cap; p++) CHECK(hit[(size_t)p] == 1);
        }
    }
    printf("combos=%lld blocks=%lld positions=%lld bad=%lld\n", combos, blocks, positions, g_bad);
    return g_bad == 0 ? 0 : 1;
}
