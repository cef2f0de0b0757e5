// tb_spmv_planners.hpp — the planning half of the SpMV unit (tb_spmv.hip): pure host functions from a CSR pattern to the arrays its product kernels read.
// Standard library only, no device, no environment, no global state: the *_plan functions of tb_spmv.hip read the environment, call these and upload
// what they return; tests/planner_driver.cpp (case `spmv`) calls them without a GPU.
#pragma once
#include <cstdint>
#include <vector>

#include "tb_planners.hpp"

namespace tb {

// one slice of the sliced mirror (k_mirror_fill, k_spmv_mirror): {first value, first column offset or −1, signature shared by its 64 rows or MIXED, width}
struct MirrorSlice { int64_t base, obase; uint32_t sig, width; uint32_t pad[2]; }; // 32 bytes
constexpr uint32_t MIRROR_MIXED = 0xFFFFFFFFu;
constexpr int32_t MIRROR_NONE = INT32_MIN; // column offset of a padding entry

namespace plan {

inline int64_t nnz_of(const PatternView &p) { return p.rowptr[p.n_rows]; }

// Is the pattern a CSR of 3×3 blocks — rows 3R, 3R+1, 3R+2 of equal length over the same columns, the columns in triples 3C, 3C+1, 3C+2, every node
// row starting at a multiple of nine?  Yes: bcol holds one column (node) index per block, nnz / 9 of them.
bool block3_columns(const PatternView &p, std::vector<int32_t> &bcol);

// Row runs of the stream kernels: greedy cuts of the row sequence at ≤ cap − 2 entries (the 16-byte value loads of k_spmv_sig_rows start one entry
// early and end one late) and ≤ 60000 rows (the record holds 16 bits of row count).  One 16-byte record per run: first row, rows | entries << 16,
// first nz (low, high word).  A pattern without rows is one empty run.  false: a single row exceeds cap − 2 (rec is left empty).
bool row_runs(const PatternView &p, int cap, std::vector<uint32_t> &rec);

// Signatures of the index-compressed product: rows with the same list of column offsets (colidx[k] − row) share one table entry.  Per row a 64-bit
// hash (parallel), de-duplication in row order with the neighbouring row as the fast path (consecutive rows of a finite-element numbering nearly
// always repeat the signature); equal hashes are told apart by length and content.  rowsig[r]: position of row r's signature in the table; the table
// ends in SIG_SLACK zeros (the kernel reads offset 0 of a row's signature for its masked entries, and whole triples).  false — the pattern does not
// compress: the table would exceed `budget` entries (an unstructured numbering: every row its own signature), the pattern is empty, or a table
// position would not fit 32 bits.
constexpr int SIG_SLACK = 32;
struct SigHost { int64_t n_sig = 0; std::vector<uint32_t> rowsig; std::vector<int32_t> tab; };
bool row_signatures(const PatternView &p, int64_t budget, SigHost &out);

// Slices of the sliced mirror: 64 consecutive rows, zero-padded to the longest row of the slice.  One record per slice and a terminator.  A full slice of one signature needs no per-row metadata; a mixed slice
// carries its column offsets entry-major like the values (4 B per entry, padding marked NONE).  rowsig: the signature plan's, or nullptr for a pattern
// without one (every slice is then mixed).  false — no mirror: a slice is wider than 255 entries.
struct MirrorHost { int64_t entries = 0; std::vector<MirrorSlice> slices; std::vector<int32_t> offs; }; // entries: Σ 64 · width; offs: never empty (one 0 when no slice is mixed)
bool mirror_slices(const PatternView &p, const uint32_t *rowsig, MirrorHost &out);

// nz index of every row's diagonal entry, −1 where none is stored
std::vector<int64_t> diagonal_positions(const PatternView &p);

} // namespace plan
} // namespace tb
