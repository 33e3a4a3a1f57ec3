// fsq_kb_tilemap.h - the step round's input lists and the map "block index -> (list, tile, count)" of its one launch.
//
// The step round (kB_step, fsq_fit_rounds.hip) runs one fit per lane and a wave waits for its slowest lane, so the fits
// are kept apart by the number of Newton iterations lmpar took for them LAST time (the count is sticky per fit, DESIGN.md
// 4.2): queue B holds four lists, and the fits parked in the middle of lmpar wait in the two lists of queue C.  Two lists
// share one array, one growing from position 0 upwards and one from cap - 1 downwards; queue B has two such arrays.
//   list       history          array              grows
//   KB_B0      <= 0 (fresh)     B, first array     up
//   KB_B1      1                B, first array     down
//   KB_B3      2 .. 4           B, second array    up
//   KB_B10     >= 5             B, second array    down
//   KB_C1      parked early     C                  up
//   KB_C3      parked late      C                  down
// Plain C++ without a device call in it: the kernel and tests/kb_tilemap_check.cpp (a host program) compile the same text.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSQ_KB_FN __host__ __device__ inline
#else
#define FSQ_KB_FN inline
#endif

enum { KB_B0 = 0, KB_B1 = 1, KB_B3 = 2, KB_B10 = 3, KB_C1 = 4, KB_C3 = 5, KB_LISTS = 6 };
enum { KB_TILE = 64 };      // fits per tile = lanes per wave

// the queue-B list of a fit whose last lmpar call took `hist` Newton iterations in all
FSQ_KB_FN int kb_list_of_history(int hist) { return hist <= 0 ? KB_B0 : hist == 1 ? KB_B1 : hist <= 4 ? KB_B3 : KB_B10; }
// which of queue B's two arrays a B list lives in, and whether a list grows downwards from cap - 1
FSQ_KB_FN int kb_list_array(int list) { return list == KB_B3 || list == KB_B10; }
FSQ_KB_FN bool kb_list_down(int list) { return (list & 1) != 0; }
// position of the list's element p in its array of cap positions
FSQ_KB_FN long long kb_list_pos(int list, long long p, long long cap) { return kb_list_down(list) ? cap - 1 - p : p; }

FSQ_KB_FN int kb_tiles(int n) { return n / KB_TILE + (n % KB_TILE != 0); }       // (no n + 63: n may be close to INT_MAX)

// Launch order: the long-running kinds first - fits parked late (they run to the end), B10, fits parked early, B3, B1, B0.
FSQ_KB_FN int kb_launch_order(int k)
{
    return k == 0 ? KB_C3 : k == 1 ? KB_B10 : k == 2 ? KB_C1 : k == 3 ? KB_B3 : k == 4 ? KB_B1 : KB_B0;
}

struct KbTile { int list, tile, count; };       // list < 0: the block has nothing to do

// n[l] = fits in list l.  Block b works on positions tile * 64 .. min(tile * 64 + 64, count) - 1 of list `list`.
FSQ_KB_FN KbTile kb_tile_of_block(long long block, const int* n)
{
    KbTile t; t.list = -1; t.tile = 0; t.count = 0;
    if (block < 0) return t;
    for (int k = 0; k < KB_LISTS; k++) {
        const int l = kb_launch_order(k);
        const int tiles = n[l] > 0 ? kb_tiles(n[l]) : 0;
        if (block < tiles) { t.list = l; t.tile = (int)block; t.count = n[l]; return t; }
        block -= tiles;
    }
    return t;
}

// blocks a launch needs for `alive` fits spread over the lists in any way: every list may end in a partial tile
FSQ_KB_FN long long kb_grid_for(long long alive) { return alive / KB_TILE + (alive % KB_TILE != 0) + KB_LISTS; }
