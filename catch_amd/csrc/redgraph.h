// What the two all-pairs files share: the pair tile, the device-resident graph (catchhip_redgraph) and the way from
// an adjacency bitmap to its CSR form.  redundant.hip owns the kernels of that way and everything that reads a graph
// (fetch, naive pass, rows, destroy); cross.hip builds graphs of its own predicate through the same way.
#pragma once
#include "internal.h"

#define RG_TILE 64
#define RG_BLOCK 256
#define RG_MAXLEN 256          // bases per probe: W = 4 words per plane

struct catchhip_redgraph {
    catchhip_ctx *ctx = nullptr;
    i64 n = 0;
    i64 nedges = 0;          // directed: every undirected pair counts twice
    DevBuf<i64> ptr;         // n + 1
    DevBuf<u32> idx;         // nedges, every row ascending
};

// The graph of G->n >= 1 vertices (G->ptr allocated) out of its adjacency bitmap (row i: `tiles` words, bit j of the
// row set iff i and j are neighbours) on ctx->stream, behind the kernels that wrote the bitmap: degrees (deg: n
// words of scratch), their scan, one read-back of the edge count, the neighbour lists.  Counts its three launches on
// `timer`, stops it and reads it after the final synchronisation.
int chip_redgraph_from_bitmap(catchhip_ctx *ctx, PhaseTimer &timer, const unsigned long long *bitmap, i64 tiles, u32 *deg,
                              catchhip_redgraph *G);
