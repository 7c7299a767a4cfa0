// Host side of the aggregation family (the extern "C" entry points of segsum.hip and gat.hip): ONE description of what such a call
// receives, ONE check of what every member requires, ONE start of the kernel's parameter block.  An entry point packs its
// arguments into a SegCall; its body states what differs (SegNeeds), runs seg_check, takes seg_params and sets only the fields of
// its own mode.
#pragma once
#include "segsum.h"
#include "draw.h"

namespace npi {

// the arguments of Rule D as the C ABI takes them
struct DropArgs { const int32_t* eid; int64_t key; uint64_t threshold; float scale; };

struct SegCall {
    const char* who;                 // the extern "C" function that was called: every message starts with it
    hipStream_t stream;
    // the CSR side (rowidx / item_row / item_edges: null / 0 where the member takes none)
    const int32_t* rowptr = nullptr; const int32_t* col = nullptr; const int32_t* rowidx = nullptr; const int32_t* item_row = nullptr;
    int64_t item_edges = 0, N = 0, nnz_max = 0;
    // the gathered table: entries with col >= split read row (col - split) of x2 when x2 is given
    const float* x = nullptr; int64_t ldx = 0; const float* x2 = nullptr; int64_t split = 0;
    // the finished rows
    float* out = nullptr; int64_t ldo = 0; float* carry = nullptr; float* row_scales_out = nullptr;
    const float* bias = nullptr;
    const DropArgs* drop = nullptr;  // Rule D (null: no attention dropout)

    SegCall(const char* who_, void* stream_) : who(who_), stream((hipStream_t)stream_) {}
    // the three groups in the order the C ABI lists them (x / out: void* where the entry point stores bf16 too)
    SegCall& side(const int32_t* rowptr_, const int32_t* col_, const int32_t* rowidx_, const int32_t* item_row_, int64_t item_edges_,
                  int64_t N_, int64_t nnz_max_) {
        rowptr = rowptr_, col = col_, rowidx = rowidx_, item_row = item_row_, item_edges = item_edges_, N = N_, nnz_max = nnz_max_;
        return *this;
    }
    SegCall& table(const void* x_, int64_t ldx_, const void* x2_, int64_t split_) {
        return x = (const float*)x_, ldx = ldx_, x2 = (const float*)x2_, split = split_, *this;
    }
    SegCall& rows(void* out_, int64_t ldo_, float* carry_, float* row_scales_out_, const float* bias_) {
        return out = (float*)out_, ldo = ldo_, carry = carry_, row_scales_out = row_scales_out_, bias = bias_, *this;
    }
};

// a condition of the call `c`; its failure ends the entry point with NPI_ERR_ARG and a message that starts with c.who
#define NPI_SEG_REQUIRE(c, cond, msg) \
    do { if (!(cond)) { npi::set_error("%s: " msg, (c).who); return NPI_ERR_ARG; } } while (0)

// the split of a two-part table and the signs of the sizes (empty_ok: a side without an entry is served)
inline int seg_check_sizes(const SegCall& c, bool empty_ok) {
    NPI_SEG_REQUIRE(c, c.x2 == nullptr || (c.split >= 0 && c.split < 0x7fffffff), "bad split");
    NPI_SEG_REQUIRE(c, c.N >= 0 && (empty_ok ? c.nnz_max >= 0 : c.nnz_max > 0), "bad size");
    return NPI_OK;
}
// the side and the table are there (col: only where there are entries)
inline bool seg_side_present(const SegCall& c, bool need_rowidx) {
    return c.rowptr && (c.col || c.nnz_max == 0) && (c.rowidx || !need_rowidx) && c.x;
}
inline bool seg_rows16(const SegCall& c) {
    return c.ldx % 4 == 0 && c.ldo % 4 == 0 && ((uintptr_t)c.x % 16) == 0 && ((uintptr_t)c.out % 16) == 0 &&
           (c.x2 == nullptr || ((uintptr_t)c.x2 % 16) == 0);
}

// what differs between the members that end in segsum_run
struct SegNeeds {
    int64_t F;                // row width: both pitches cover it
    bool rowidx = false;      // the mode reads the side's rowidx
    bool empty_ok = false;    // nnz_max == 0 is served
    int64_t scales_F = 0;     // row_scales_out is served at this row width alone (0: not at all)
    bool rows16 = false;      // the several-head modes: 16-byte rows and carry (one head: whatever segsum_run's vector pick serves)
};

constexpr int SEG_PROCEED = 1;
// SEG_PROCEED, or the status the entry point returns at once: NPI_ERR_ARG (message set), NPI_OK for N == 0 (no pointer examined)
inline int seg_check(const SegCall& c, const SegNeeds& n) {
    NPI_SEG_REQUIRE(c, item_edges_ok(c.item_edges), "item_edges must be 64 or NPI_ITEM_EDGES (the value the CSR was built with)");
    if (const int rc = seg_check_sizes(c, n.empty_ok); rc != NPI_OK) return rc;
    NPI_SEG_REQUIRE(c, c.row_scales_out == nullptr || (n.scales_F != 0 && n.F == n.scales_F && seg_rows16(c)),
                    "row_scales_out needs f32 rows of 256 columns, 16-byte aligned, one head or the fused backward, and a graph with entries");
    if (c.N == 0) return NPI_OK;
    NPI_SEG_REQUIRE(c, seg_side_present(c, n.rowidx) && c.item_row && c.out && c.carry, "null pointer");
    NPI_SEG_REQUIRE(c, c.ldx >= n.F && c.ldo >= n.F, "leading dimension too small");
    NPI_SEG_REQUIRE(c, !n.rows16 || (seg_rows16(c) && ((uintptr_t)c.carry % 16) == 0), "several heads need 16-byte aligned rows and carry");
    NPI_SEG_REQUIRE(c, c.drop == nullptr || c.drop->eid != nullptr, "null eid (attention dropout is keyed on the entries' edge ids)");
    return SEG_PROCEED;
}

// the parameter block with everything the call describes filled in; the body adds the fields of its mode
inline SegParams seg_params(const SegCall& c, int64_t F) {
    SegParams P{};
    P.rowptr = c.rowptr; P.col = c.col; P.item_row = c.item_row; P.rowidx = c.rowidx;
    P.N = (int)c.N; P.item = (int)c.item_edges;
    P.x = c.x; P.ldx = c.ldx; P.out = c.out; P.ldo = c.ldo; P.F = (int)F;
    P.x2 = c.x2; P.split = (int)c.split;
    P.carry = c.carry; P.bias = c.bias;
    P.scale_out = c.row_scales_out;
    if (c.drop != nullptr) {
        P.eid = c.drop->eid;
        P.drop_root = draw_root(c.drop->key, DRAW_RULE_D);
        P.drop_threshold = c.drop->threshold;
        P.drop_scale = c.drop->scale;
    }
    return P;
}

}  // namespace npi
