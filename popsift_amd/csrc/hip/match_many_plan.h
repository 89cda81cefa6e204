// match_many_plan.h -- the tables of the one-to-many byte pair search (psx_match_pairs_many_u8, include/popsift_hip.h):
// which rows every workgroup of k_match_u8_many (match_many.hip) takes on its outer and on its inner side.
//
// Plain C++14, no HIP: match_many.hip builds its device tables with these functions, psx_match_many_plan hands them
// out, and a stand-alone program can include the header alone (tests/cpp/match_many_plan_san.cpp).
//
// A SIDE is a list of sets (lengths >= 0).  It is cut two ways:
//   inner chunks {set, r0, r1}: rows [r0, r1) of one set, r0 a multiple of 32 (whole MFMA tiles), r1 - r0 <= 512 (the 9
//                  index bits of the matcher's key); a set's chunks are ascending and contiguous in the table
//   outer blocks {set, row0}:   rows [row0, min(row0 + 256, len)) of one set: what one workgroup holds as MFMA columns
// Every row of every non-empty set is covered exactly once by either table, nothing spans two sets, empty sets
// contribute nothing.  The forward direction pairs the blocks of {L} with the chunks of the K right sets, the backward
// direction the blocks of the K right sets with the chunks of {L}.
#pragma once

#include "popsift_hip.h"

constexpr int PSX_MANY_TILE = 32;            // rows per MFMA tile
constexpr int PSX_MANY_CHUNK_MAX = 512;      // rows per chunk: 9 index bits in the key
constexpr int PSX_MANY_BLOCK = 256;          // outer rows per workgroup
constexpr int PSX_MANY_WGS = 2048;           // workgroups a pass aims at, as u8_plan (match.hip) does: 256 CUs x 4 SIMDs x 2

// blocks of a side; out may be NULL (count only), nothing is written at or past cap
inline long long psx_many_blocks(const int* lens, int n, psx_many_block* out, long long cap)
{
    long long c = 0;
    for (int s = 0; s < n; s++)
        for (long long row0 = 0; row0 < lens[s]; row0 += PSX_MANY_BLOCK, c++)
            if (out != nullptr && c < cap) { out[c].set = s; out[c].row0 = (int)row0; }
    return c;
}

// The chunk length of a side whose other side has outer_blocks blocks: as u8_plan chooses it for one set -- enough
// (block, chunk) workgroups for the chip, whole tiles, at most 512 rows -- with the rows of ALL sets in the sum.
inline int psx_many_chunk_len(const int* lens, int n, long long outer_blocks)
{
    long long rows = 0;
    for (int s = 0; s < n; s++) rows += lens[s];
    if (outer_blocks < 1) outer_blocks = 1;
    const long long want = (PSX_MANY_WGS + outer_blocks - 1) / outer_blocks;          // chunks, over all sets
    long long len = (rows + want - 1) / want;
    len = ((len + PSX_MANY_TILE - 1) / PSX_MANY_TILE) * PSX_MANY_TILE;
    if (len < PSX_MANY_TILE) len = PSX_MANY_TILE;
    if (len > PSX_MANY_CHUNK_MAX) len = PSX_MANY_CHUNK_MAX;
    return (int)len;
}

// chunks of a side at a given chunk length (whole tiles, <= 512): every set is cut into ceil(len / target) chunks of equal
// length (whole tiles), so a set slightly longer than target gives two halves, not one full chunk and a sliver
inline long long psx_many_chunks_of(const int* lens, int n, int target, psx_many_chunk* out, long long cap)
{
    long long c = 0;
    for (int s = 0; s < n; s++) {
        const long long len = lens[s];
        if (len <= 0) continue;
        const long long pieces = (len + target - 1) / target;
        long long step = (len + pieces - 1) / pieces;
        step = ((step + PSX_MANY_TILE - 1) / PSX_MANY_TILE) * PSX_MANY_TILE;          // <= target: target is whole tiles
        for (long long r0 = 0; r0 < len; r0 += step, c++)
            if (out != nullptr && c < cap) {
                out[c].set = s; out[c].r0 = (int)r0; out[c].r1 = (int)(r0 + step < len ? r0 + step : len);
            }
    }
    return c;
}

// chunks of a side whose other side has outer_blocks blocks: at the length psx_many_chunk_len chooses
inline long long psx_many_chunks(const int* lens, int n, long long outer_blocks, psx_many_chunk* out, long long cap)
{
    return psx_many_chunks_of(lens, n, psx_many_chunk_len(lens, n, outer_blocks), out, cap);
}

// what every one-to-many entry point refuses about its sets, before anything else is looked at
inline bool psx_many_sets_ok(int l_len, const int* r_lens, int n_sets)
{
    if (l_len < 0 || n_sets < 0 || (n_sets > 0 && r_lens == nullptr)) return false;
    long long rows = 0;
    for (int k = 0; k < n_sets; k++) {
        if (r_lens[k] < 0) return false;
        rows += r_lens[k];
    }
    return rows <= 2147483647LL && (long long)n_sets * l_len <= 2147483647LL;
}

// psx_match_many_plan (include/popsift_hip.h): one direction's two tables
inline int psx_many_plan_host(int l_len, const int* r_lens, int n_sets, int backward,
                              psx_many_chunk* chunks, int chunk_capacity, int* chunk_count,
                              psx_many_block* blocks, int block_capacity, int* block_count)
{
    if (!psx_many_sets_ok(l_len, r_lens, n_sets) || chunk_count == nullptr || block_count == nullptr ||
        chunk_capacity < 0 || block_capacity < 0 || (chunk_capacity > 0 && chunks == nullptr) ||
        (block_capacity > 0 && blocks == nullptr) || (backward != 0 && backward != 1))
        return PSX_ERR_INVALID;
    const int* outer = backward ? r_lens : &l_len;
    const int* inner = backward ? &l_len : r_lens;
    const int n_outer = backward ? n_sets : 1, n_inner = backward ? 1 : n_sets;
    const long long nb = psx_many_blocks(outer, n_outer, blocks, block_capacity);
    const long long nc = psx_many_chunks(inner, n_inner, nb, chunks, chunk_capacity);
    *block_count = (int)nb;                  // <= rows / 256 + sets, rows / 32 + sets: both fit (psx_many_sets_ok)
    *chunk_count = (int)nc;
    return PSX_OK;
}
