// s2k.hpp -- header-only C++17 facade over the C ABI (s2k.h) with the reference's interface shape:
//   s2k::KminmersIterator(seq, l, k, density, mode)  ~  KminmersIterator::new      src/lib.rs:89-131
//   range-for over it yields s2k::KminmerHash           ~  impl Iterator             src/lib.rs:179-270
//   s2k::KminmerHash{hash,start,end,offset,rev}, == / < by hash only               src/kminmer.rs:128-135,181-204
//   s2k::HashMode                                                                    src/lib.rs:21-27
//   s2k::NtHashHPCIterator / NtHashSIMDIterator / NtHashHPCSIMDIterator (seq, l, hash_bound)   src/lib.rs:6-13 (re-exports)
// Parameter violations that panic in the reference throw s2k::Error here.  The efficient entry point is
// Engine::extract (a batch of reads per call); the per-read iterator exists for reference-style call sites.
#pragma once
#include "s2k.h"

#include <cstdint>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

namespace s2k {

enum class HashMode : int32_t { Regular = S2K_MODE_REGULAR, Hpc = S2K_MODE_HPC, Simd = S2K_MODE_SIMD, HpcSimd = S2K_MODE_HPCSIMD };

struct Error : std::runtime_error {
    s2k_status status;
    Error(s2k_status st, const std::string &what) : std::runtime_error(what), status(st) {}
};

struct KminmerHash { // src/kminmer.rs:128-135
    uint64_t hash;
    size_t start, end, offset;
    bool rev;
    uint64_t get_hash() const { return hash; }                                      // src/kminmer.rs:162-164
    friend bool operator==(const KminmerHash &a, const KminmerHash &b) { return a.hash == b.hash; } // :181-185
    friend bool operator<(const KminmerHash &a, const KminmerHash &b) { return a.hash < b.hash; }    // :194-198
};

class Batch { // owns one s2k_result
  public:
    Batch() { res_ = s2k_result{}; }
    Batch(const Batch &) = delete;
    Batch &operator=(const Batch &) = delete;
    Batch(Batch &&o) noexcept : res_(o.res_) { o.res_ = s2k_result{}; }
    Batch &operator=(Batch &&o) noexcept {
        if (this != &o) {
            s2k_result_free(&res_);
            res_ = o.res_;
            o.res_ = s2k_result{};
        }
        return *this;
    }
    ~Batch() { s2k_result_free(&res_); }
    uint64_t n_reads() const { return res_.n_reads; }
    uint64_t n_kminmers() const { return res_.n_kminmers; }
    uint64_t begin_of(uint64_t r) const { return res_.km_off[r]; }
    uint64_t end_of(uint64_t r) const { return res_.km_off[r + 1]; }
    KminmerHash item(uint64_t r, uint64_t i) const { // i-th k-min-mer of read r
        uint64_t g = res_.km_off[r] + i;
        return KminmerHash{res_.hash[g], res_.start[g], res_.end[g], (size_t)i, res_.rev[g] != 0};
    }
    uint64_t n_minimizers() const { return res_.n_minimizers; } // with S2K_FLAG_WANT_MINIMIZERS
    const s2k_result &raw() const { return res_; }
    s2k_result *out() { return &res_; }

  private:
    s2k_result res_;
};

class Engine { // one per thread and device (like one KminmersIterator per thread, src/main.rs:65-79)
  public:
    explicit Engine(int device = 0) {
        s2k_status st;
        ctx_ = s2k_create(device, &st);
        if (!ctx_) throw Error(st, std::string("s2k_create: ") + s2k_strerror(st));
    }
    Engine(const Engine &) = delete;
    Engine &operator=(const Engine &) = delete;
    ~Engine() { s2k_destroy(ctx_); }

    // double buffering with two engines on one device (s2k_chain_after): this engine's minimizer kernels wait for those of prev's most recent
    // call; chain both ways, alternate the calls from one thread; nullptr unlinks (do so before prev is destroyed)
    void chain_after(Engine *prev) {
        s2k_status st = s2k_chain_after(ctx_, prev ? prev->ctx_ : nullptr);
        if (st != S2K_OK) throw Error(st, s2k_strerror(st));
    }
    // bases per sub-batch of extract(): H2D / kernels / D2H of consecutive sub-batches overlap (0 = default, 2^29)
    void set_host_batch(uint64_t bases) {
        s2k_status st = s2k_set_host_batch(ctx_, bases);
        if (st != S2K_OK) throw Error(st, s2k_strerror(st));
    }
    Batch extract(const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads, size_t l, size_t k, double density,
                  HashMode mode, uint32_t flags = 0) {
        s2k_params p{(uint32_t)l, (uint32_t)k, density, (int32_t)mode, flags};
        Batch b;
        s2k_status st = s2k_extract(ctx_, bases, read_off, n_reads, &p, b.out());
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return b;
    }
    Batch extract(const std::vector<std::string_view> &reads, size_t l, size_t k, double density, HashMode mode, uint32_t flags = 0) {
        std::vector<uint64_t> off(reads.size() + 1, 0);
        std::string bases;
        for (size_t i = 0; i < reads.size(); i++) {
            bases.append(reads[i]);
            off[i + 1] = bases.size();
        }
        return extract(reinterpret_cast<const uint8_t *>(bases.data()), off.data(), reads.size(), l, k, density, mode, flags);
    }
    // s2k_count_device_ex on device-resident hashes: the pairs of the keys that occur >= min_count times, in ascending key order when
    // `sorted`; d_keys / d_counts may be nullptr (sizes only).  Throws Error(S2K_ERR_CAPACITY) when n_kept > capacity.
    struct CountSizes {
        uint64_t n_distinct, n_kept;
    };
    CountSizes count_device(const uint64_t *d_hash, uint64_t n, uint32_t min_count, bool sorted, uint64_t *d_keys = nullptr,
                            uint32_t *d_counts = nullptr, uint64_t capacity = 0) {
        CountSizes r{0, 0};
        s2k_status st = s2k_count_device_ex(ctx_, d_hash, n, min_count, sorted ? S2K_COUNT_SORTED : 0u, d_keys, d_counts, capacity,
                                            &r.n_distinct, &r.n_kept);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return r;
    }
    // s2k_count_merge_device: the union of two strictly ascending count tables, counts added (saturated), pairs under min_count
    // dropped; d_keys / d_counts may be nullptr (sizes only).  Throws Error(S2K_ERR_CAPACITY) when n_kept > capacity.
    CountSizes count_merge(const uint64_t *d_a_keys, const uint32_t *d_a_counts, uint64_t n_a, const uint64_t *d_b_keys,
                           const uint32_t *d_b_counts, uint64_t n_b, uint32_t min_count, uint64_t *d_keys = nullptr,
                           uint32_t *d_counts = nullptr, uint64_t capacity = 0) {
        CountSizes r{0, 0};
        s2k_status st = s2k_count_merge_device(ctx_, d_a_keys, d_a_counts, n_a, d_b_keys, d_b_counts, n_b, min_count, d_keys, d_counts,
                                               capacity, &r.n_distinct, &r.n_kept);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return r;
    }
    // s2k_run_file_count: the file mode, each batch's k-min-mer hashes added to `counter` (a Counter of an engine on this device)
    s2k_counts run_file_count(const char *path, const s2k_params &params, uint64_t batch_bases, s2k_counter *counter,
                              double *seconds = nullptr) {
        s2k_counts tot{};
        s2k_status st = s2k_run_file_count(ctx_, path, &params, batch_bases, counter, &tot, seconds);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return tot;
    }
    // s2k_graph_adjacency: the CSR over 2 * n_nodes oriented nodes from strictly ascending edge keys (u << 32 | v); d_row_off holds
    // 2 * n_nodes + 1 entries, d_dst (may be nullptr) n_edges.  Throws Error(S2K_ERR_INVALID_ARG) for keys that break the rules.
    void graph_adjacency(const uint64_t *d_edge_keys, uint64_t n_edges, uint64_t n_nodes, uint64_t *d_row_off, uint32_t *d_dst = nullptr) {
        s2k_status st = s2k_graph_adjacency(ctx_, d_edge_keys, n_edges, n_nodes, d_row_off, d_dst);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
    }
    // s2k_graph_unitigs: the non-branching paths of a twin-symmetric CSR compacted; out (may be nullptr: sizes only) names the device
    // arrays to fill.  Returns the number of unitigs, *n_links (may be nullptr) the number of oriented nodes with a next.  Throws
    // Error(S2K_ERR_INVALID_ARG) for a CSR that breaks the rules or lacks a twin, Error(S2K_ERR_CAPACITY) when out->capacity is short.
    uint64_t graph_unitigs(const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_nodes, const s2k_unitig_out *out,
                           uint64_t *n_links = nullptr) {
        uint64_t n_unitigs = 0, links = 0;
        s2k_status st = s2k_graph_unitigs(ctx_, d_row_off, d_dst, n_edges, n_nodes, out, &n_unitigs, &links);
        if (n_links) *n_links = links;
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_unitigs;
    }
    // s2k_graph_unitig_edges: the keys U << 32 | V between the oriented unitigs, strictly ascending, and (d_src_edge, may be nullptr)
    // the CSR edge each came from; the unitig arrays are those graph_unitigs wrote for the same CSR.  Returns the number of keys
    // (d_keys nullptr: the size only).
    uint64_t graph_unitig_edges(const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_nodes, const uint64_t *d_uni_off,
                                const uint32_t *d_members, const uint32_t *d_node_unitig, const uint32_t *d_node_pos, uint64_t n_unitigs,
                                uint64_t *d_keys, uint64_t *d_src_edge, uint64_t capacity) {
        uint64_t n_out = 0;
        s2k_status st = s2k_graph_unitig_edges(ctx_, d_row_off, d_dst, n_edges, n_nodes, d_uni_off, d_members, d_node_unitig, d_node_pos, n_unitigs,
                                               d_keys, d_src_edge, capacity, &n_out);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_out;
    }
    // s2k_graph_simplify_mask: one round of tip clipping and simple-bubble popping on the unitig graph (CSR over 2 * n_unitigs oriented
    // unitigs, d_uni_off, d_uni_count = the summed node counts); d_remove (one byte per unitig) may be nullptr: the totals only.
    struct SimplifyTotals {
        uint64_t tips, bubbles, removed;
    };
    SimplifyTotals graph_simplify_mask(const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                       const uint64_t *d_uni_off, const uint64_t *d_uni_count, uint32_t max_tip, uint32_t max_bubble,
                                       uint8_t *d_remove) {
        SimplifyTotals t{};
        s2k_status st = s2k_graph_simplify_mask(ctx_, d_row_off, d_dst, n_edges, n_unitigs, d_uni_off, d_uni_count, max_tip, max_bubble, d_remove,
                                                &t.tips, &t.bubbles, &t.removed);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_graph_bubble_mask: one round of bounded superbubble popping on the same unitig graph (the rule is in s2k.h): an interior of at
    // most max_nodes unitigs (1 .. S2K_BUBBLE_MAX_NODES) and max_bubble members; d_remove (one byte per unitig) may be nullptr: the totals only.
    struct BubbleTotals {
        uint64_t sources, found, applied, removed;
    };
    BubbleTotals graph_bubble_mask(const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs, const uint64_t *d_uni_off,
                                   const uint64_t *d_uni_count, uint32_t max_nodes, uint32_t max_bubble, uint8_t *d_remove) {
        BubbleTotals t{};
        s2k_status st = s2k_graph_bubble_mask(ctx_, d_row_off, d_dst, n_edges, n_unitigs, d_uni_off, d_uni_count, max_nodes, max_bubble, d_remove,
                                              &t.sources, &t.found, &t.applied, &t.removed);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_graph_induced: the subgraph of the kept nodes.  Kept = d_node_keep[i] != 0, or (d_node_keep nullptr) !d_remove[d_node_unitig[i]].
    // Every output may be nullptr (all: the sizes only).  Returns {nodes, edges} kept; throws on S2K_ERR_CAPACITY too (nothing written).
    struct InducedSizes {
        uint64_t nodes, edges;
    };
    InducedSizes graph_induced(const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n_nodes, const uint64_t *d_edge_keys,
                               const uint32_t *d_edge_counts, uint64_t n_edges, const uint8_t *d_node_keep, const uint32_t *d_node_unitig,
                               const uint8_t *d_remove, uint64_t n_unitigs, uint32_t *d_new_id, uint64_t *d_keys_out, uint32_t *d_counts_out,
                               uint64_t node_capacity, uint64_t *d_edge_keys_out, uint32_t *d_edge_counts_out, uint64_t edge_capacity) {
        InducedSizes n{};
        s2k_status st = s2k_graph_induced(ctx_, d_keys, d_counts, n_nodes, d_edge_keys, d_edge_counts, n_edges, d_node_keep, d_node_unitig, d_remove,
                                          n_unitigs, d_new_id, d_keys_out, d_counts_out, node_capacity, d_edge_keys_out, d_edge_counts_out,
                                          edge_capacity, &n.nodes, &n.edges);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n;
    }
    // s2k_unitig_sequences: the unitigs' base-space sequences stitched from the node records (s2k_node_seqs, filled by
    // Table::node_sequences); d_out_off (n_unitigs + 1), d_out (16-byte aligned) and d_overlap (2 * n_unitigs) may each be nullptr.
    // Returns the number of bases (throws on S2K_ERR_CAPACITY too: nothing is written then).
    uint64_t unitig_sequences(const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular, uint64_t n_unitigs, uint64_t n_nodes,
                              const s2k_node_seqs &nodes, uint64_t *d_out_off, uint8_t *d_out = nullptr, uint64_t capacity = 0,
                              uint32_t *d_overlap = nullptr) {
        uint64_t n_bases = 0;
        s2k_status st = s2k_unitig_sequences(ctx_, d_uni_off, d_members, d_circular, n_unitigs, n_nodes, &nodes, d_out_off, d_out, d_overlap, capacity,
                                             &n_bases);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_bases;
    }
    // s2k_unitig_node_places: d_place[i] (n_nodes 16-byte records) = where node i lies on the oriented unitigs, from the arrays
    // graph_unitigs wrote.  Throws Error(S2K_ERR_INVALID_ARG) for arrays that are not a decomposition of the n_nodes nodes.
    void unitig_node_places(const uint64_t *d_uni_off, const uint32_t *d_members, const uint32_t *d_node_unitig, const uint32_t *d_node_pos,
                            const uint8_t *d_circular, uint64_t n_nodes, uint64_t n_unitigs, s2k_node_place *d_place) {
        s2k_status st = s2k_unitig_node_places(ctx_, d_uni_off, d_members, d_node_unitig, d_node_pos, d_circular, n_nodes, n_unitigs, d_place);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
    }
    // s2k_paths_spans: the span keys of the paths of one batch (the arrays of Table::thread) over the CSR of the oriented unitigs; d_span_keys
    // nullptr: the sizes only; d_edge_support (may be nullptr, one uint64_t per edge) gains the steps that follow every edge and its twin.
    // Throws on S2K_ERR_CAPACITY too (nothing written).
    struct SpanTotals {
        uint64_t keys, followed, off_graph;
    };
    SpanTotals paths_spans(uint64_t n_reads, const s2k_thread_out &paths, uint64_t n_steps, const uint64_t *d_row_off, const uint32_t *d_dst,
                           uint64_t n_edges, const uint64_t *d_uni_off, uint64_t n_unitigs, uint64_t *d_span_keys = nullptr, uint64_t capacity = 0,
                           uint64_t *d_edge_support = nullptr) {
        SpanTotals t{};
        s2k_status st = s2k_paths_spans(ctx_, n_reads, &paths, n_steps, d_row_off, d_dst, n_edges, d_uni_off, n_unitigs, d_span_keys, capacity,
                                        d_edge_support, &t.keys, &t.followed, &t.off_graph);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_graph_resolve_mask: the unitigs whose in- and out-edges a span table (keys strictly ascending, counts) pairs one to one;
    // d_resolved (one byte per unitig) and d_partner (one uint32_t per edge, S2K_NO_PARTNER where there is none) may be nullptr.
    struct ResolveTotals {
        uint64_t candidates, resolved;
    };
    ResolveTotals graph_resolve_mask(const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                     const uint64_t *d_span_keys, const uint32_t *d_span_counts, uint64_t n_spans, uint32_t min_support,
                                     uint8_t *d_resolved, uint32_t *d_partner) {
        ResolveTotals t{};
        s2k_status st = s2k_graph_resolve_mask(ctx_, d_row_off, d_dst, n_edges, n_unitigs, d_span_keys, d_span_counts, n_spans, min_support,
                                               d_resolved, d_partner, &t.candidates, &t.resolved);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_graph_untangle: every resolved unitig (d_resolved, d_partner of graph_resolve_mask) duplicated once per matched pair of edges:
    // d_copy_off (n_unitigs + 1), d_origin and d_copy_count (one per copy; the counts only with d_uni_count and d_edge_counts), d_keys
    // (n_edges, strictly ascending: graph_adjacency takes them over `copies` nodes) and d_src_edge; all nullptr: the sizes only.  Throws
    // on S2K_ERR_CAPACITY too (more copies than `capacity`; nothing written).
    struct UntangleTotals {
        uint64_t copies, duplicated;
    };
    UntangleTotals graph_untangle(const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs, const uint8_t *d_resolved,
                                  const uint32_t *d_partner, const uint64_t *d_uni_count = nullptr, const uint32_t *d_edge_counts = nullptr,
                                  uint64_t *d_copy_off = nullptr, uint32_t *d_origin = nullptr, uint64_t *d_copy_count = nullptr,
                                  uint64_t *d_keys = nullptr, uint64_t *d_src_edge = nullptr, uint64_t capacity = 0) {
        UntangleTotals t{};
        s2k_status st = s2k_graph_untangle(ctx_, d_row_off, d_dst, n_edges, n_unitigs, d_resolved, d_partner, d_uni_count, d_edge_counts, d_copy_off,
                                           d_origin, d_copy_count, d_keys, d_src_edge, capacity, &t.copies, &t.duplicated);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_unitig_expand: the contigs (`outer`: uni_off, members and circular of graph_unitigs over the n_copies copies; outer.capacity =
    // their number) as node members, through d_origin and the inner decomposition (`inner`, inner.capacity = n_unitigs, over n_nodes
    // nodes).  `out` receives uni_off, members, node_unitig, node_pos and circular, d_node_origin the old node of every instance;
    // out.capacity = the instances they hold.  Returns the number of instances (throws on S2K_ERR_CAPACITY too).
    uint64_t unitig_expand(const s2k_unitig_out &outer, uint64_t n_copies, const uint32_t *d_origin, const s2k_unitig_out &inner, uint64_t n_nodes,
                           const s2k_unitig_out &out, uint32_t *d_node_origin = nullptr) {
        uint64_t n_members = 0;
        s2k_status st = s2k_unitig_expand(ctx_, outer.uni_off, outer.members, outer.circular, outer.capacity, n_copies, d_origin, inner.uni_off,
                                          inner.members, inner.circular, inner.capacity, n_nodes, out.uni_off, out.members, out.node_unitig,
                                          out.node_pos, out.circular, d_node_origin, out.capacity, &n_members);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_members;
    }
    // s2k_unitig_member_offsets: where every member's piece starts in the stitched unitigs (d_member_off, n_nodes entries), with d_out_off
    // and d_overlap as unitig_sequences writes them; each may be nullptr.  Returns the bases of all unitigs.
    uint64_t unitig_member_offsets(const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular, uint64_t n_unitigs, uint64_t n_nodes,
                                   const s2k_node_seqs &nodes, uint64_t *d_member_off, uint64_t *d_out_off = nullptr, uint32_t *d_overlap = nullptr) {
        uint64_t n_bases = 0;
        s2k_status st = s2k_unitig_member_offsets(ctx_, d_uni_off, d_members, d_circular, n_unitigs, n_nodes, &nodes, d_member_off, d_out_off, d_overlap,
                                                  &n_bases);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_bases;
    }
    // s2k_paths_walks: the walks of one batch's paths along the edges of the CSR, with base coordinates (`lift`: uni_off, members and
    // circular of the decomposition, lift.capacity = n_unitigs).  out nullptr: the sizes only.  Throws on S2K_ERR_CAPACITY too (nothing
    // written).
    struct WalkTotals {
        uint64_t walks, followed, off_graph;
    };
    WalkTotals paths_walks(uint64_t n_reads, const s2k_thread_out &paths, uint64_t n_steps, const uint64_t *d_row_off, const uint32_t *d_dst,
                           uint64_t n_edges, const s2k_unitig_out &lift, uint64_t n_nodes, const uint64_t *d_member_off, const uint64_t *d_out_off,
                           const uint32_t *d_overlap, const uint32_t *d_seq_len, const s2k_walk_out *out = nullptr) {
        WalkTotals t{};
        s2k_status st = s2k_paths_walks(ctx_, n_reads, &paths, n_steps, d_row_off, d_dst, n_edges, lift.uni_off, lift.circular, lift.capacity,
                                        d_member_off, d_out_off, d_overlap, d_seq_len, lift.members, n_nodes, out, &t.walks, &t.followed, &t.off_graph);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_paths_bridge: one batch's paths with the error gaps bridged over the CSR (steps a few items apart on one unitig merged, steps a
    // few items apart across one edge extended to it; max_gap, max_slip in items).  out.path_off is required; the step arrays of `out`
    // and d_matched all nullptr: the sizes only.  d_join: one byte per input step.  Throws on S2K_ERR_CAPACITY too (nothing written).
    struct BridgeTotals {
        uint64_t steps, merged, bridged;
    };
    BridgeTotals paths_bridge(uint64_t n_reads, const s2k_thread_out &paths, uint64_t n_steps, const uint64_t *d_row_off, const uint32_t *d_dst,
                              uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular, uint64_t n_unitigs, uint32_t max_gap,
                              uint32_t max_slip, const s2k_thread_out &out, uint32_t *d_matched = nullptr, uint8_t *d_join = nullptr) {
        BridgeTotals t{};
        s2k_status st = s2k_paths_bridge(ctx_, n_reads, &paths, n_steps, d_row_off, d_dst, n_edges, d_uni_off, d_circular, n_unitigs, max_gap, max_slip,
                                         &out, d_matched, d_join, &t.steps, &t.merged, &t.bridged);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_unitig_copy_places: where the forward strand of every copy of an untangled graph lies on the oriented contigs (`outer`: uni_off,
    // members and circular of graph_unitigs over the n_copies copies; outer.capacity = their number), through d_origin and the uni_off and
    // circular of the n_unitigs unitigs the copies were made of.  d_copy_place: n_copies records, 16-byte aligned.
    void unitig_copy_places(const s2k_unitig_out &outer, uint64_t n_copies, const uint32_t *d_origin, const uint64_t *d_uni_off,
                            const uint8_t *d_circular, uint64_t n_unitigs, s2k_node_place *d_copy_place) {
        s2k_status st = s2k_unitig_copy_places(ctx_, outer.uni_off, outer.members, outer.circular, outer.capacity, n_copies, d_origin, d_uni_off,
                                               d_circular, n_unitigs, d_copy_place);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
    }
    // s2k_paths_lift: one batch's paths on the old unitig graph carried onto the contigs of its untangling (d_resolved, d_partner as
    // graph_untangle took them, d_copy_off as it wrote it, d_copy_place of unitig_copy_places).  out.path_off is required; the step
    // arrays of `out` and d_matched all nullptr: the sizes only.  d_step_copy and d_join: one entry per input step; d_contig_items:
    // n_contigs sums that accumulate.  Throws on S2K_ERR_CAPACITY too (nothing written).
    struct LiftGraph {
        const uint64_t *row_off;
        const uint32_t *dst;
        uint64_t n_edges;
        const uint64_t *uni_off;
        const uint8_t *circular;
        uint64_t n_unitigs;
        const uint8_t *resolved;
        const uint32_t *partner;
        const uint64_t *copy_off;
        const s2k_node_place *copy_place;
        uint64_t n_copies, n_contigs;
    };
    struct LiftTotals {
        uint64_t steps, merged, dropped, conflicts;
    };
    LiftTotals paths_lift(uint64_t n_reads, const s2k_thread_out &paths, uint64_t n_steps, const LiftGraph &g, const s2k_thread_out &out,
                          const uint32_t *d_matched_in = nullptr, uint32_t *d_matched = nullptr, uint32_t *d_step_copy = nullptr,
                          uint8_t *d_join = nullptr, uint64_t *d_contig_items = nullptr) {
        LiftTotals t{};
        s2k_status st = s2k_paths_lift(ctx_, n_reads, &paths, n_steps, d_matched_in, g.row_off, g.dst, g.n_edges, g.uni_off, g.circular, g.n_unitigs,
                                       g.resolved, g.partner, g.copy_off, g.copy_place, g.n_copies, g.n_contigs, &out, d_matched, d_step_copy, d_join,
                                       d_contig_items, &t.steps, &t.merged, &t.dropped, &t.conflicts);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_vote_ordinals: d_rep[i] = the ordinal packed into d_best[i] (Table::vote_representatives), all ones where d_best[i] == 0
    void vote_ordinals(const uint64_t *d_best, uint64_t n, uint64_t *d_rep) {
        s2k_status st = s2k_vote_ordinals(ctx_, d_best, n, d_rep);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
    }
    // s2k_walks_targets: the bases of every walk's path interval (`walks`: the record arrays s2k_paths_walks wrote, walks.capacity =
    // n_walks; d_step_unitig: the paths' unitig per step).  d_tgt nullptr: the sizes only.  Returns the bytes of all targets; throws on
    // S2K_ERR_CAPACITY too (nothing written).
    uint64_t walks_targets(const s2k_walk_out &walks, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off, const uint8_t *d_out,
                           uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, uint64_t *d_tgt_off = nullptr, uint8_t *d_tgt = nullptr,
                           uint8_t *d_bad = nullptr, uint64_t capacity = 0) {
        uint64_t n_bytes = 0;
        s2k_status st = s2k_walks_targets(ctx_, walks.capacity, walks.first_step, walks.n_steps, walks.path_start, walks.path_end, walks.flags, d_step_unitig,
                                          n_steps, d_out_off, d_out, n_bases, d_overlap, n_unitigs, d_tgt_off, d_tgt, d_bad, capacity, &n_bytes);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_bytes;
    }
    // s2k_align_pairs: pair i aligns d_query[q_begin[i], q_end[i]) with d_target[t_begin[i], t_end[i]) at unit costs.  out nullptr or
    // without ops, n_ops and matches: the sizes only.  Returns the run slots of all pairs; throws on S2K_ERR_CAPACITY too (nothing written).
    struct Pool {
        const uint8_t *bytes;
        uint64_t n_bytes;
        const uint64_t *begin, *end; // one interval per pair
    };
    uint64_t align_pairs(const Pool &query, const Pool &target, uint64_t n_pairs, uint32_t max_edits = S2K_ALIGN_MAX_EDITS, const s2k_align_out *out = nullptr) {
        uint64_t n_ops_bound = 0;
        s2k_status st = s2k_align_pairs(ctx_, query.bytes, query.n_bytes, target.bytes, target.n_bytes, query.begin, query.end, target.begin, target.end,
                                        n_pairs, max_edits, out, &n_ops_bound);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_ops_bound;
    }
    // s2k_walks_pileup: the aligned walks of one batch vote on the unitigs' bases (`walks` as for walks_targets; query.begin: where every
    // walk's query interval starts, query.end is not read; al: what align_pairs wrote for the walks, al.capacity = the runs d_ops holds).
    // The pile is the caller's, zeroed before the first batch.  Returns the S2K_PILEUP_STATS counters.
    struct PileupStats {
        uint64_t v[S2K_PILEUP_STATS];
    };
    PileupStats walks_pileup(const s2k_walk_out &walks, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off, const uint8_t *d_out,
                             uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, const Pool &query, const s2k_align_out &al, const s2k_pile &pile,
                             uint32_t max_shift = S2K_PILEUP_MAX_SHIFT) {
        PileupStats t{};
        s2k_status st = s2k_walks_pileup(ctx_, walks.capacity, walks.first_step, walks.n_steps, walks.path_start, walks.path_end, walks.flags, d_step_unitig,
                                         n_steps, d_out_off, d_out, n_bases, d_overlap, n_unitigs, query.bytes, query.n_bytes, query.begin, al.flags, al.ops_off,
                                         al.n_ops, al.ops, al.capacity, max_shift, &pile, t.v);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_pileup_consensus: the polished bases of every unitig.  d_new_out nullptr: the sizes only.  Returns the new bases and the
    // S2K_CONSENSUS_STATS counters; throws on S2K_ERR_CAPACITY too (nothing written).
    struct Consensus {
        uint64_t n_new_bases;
        uint64_t stats[S2K_CONSENSUS_STATS];
    };
    Consensus pileup_consensus(const s2k_pile &pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap,
                               uint64_t n_unitigs, uint32_t min_cov, uint64_t *d_new_out_off = nullptr, uint8_t *d_new_out = nullptr, uint64_t capacity = 0,
                               uint64_t *d_pos_map = nullptr, uint32_t *d_new_overlap = nullptr) {
        Consensus t{};
        s2k_status st = s2k_pileup_consensus(ctx_, &pile, d_out_off, d_out, n_bases, d_overlap, n_unitigs, min_cov, d_new_out_off, d_new_out, capacity, d_pos_map,
                                             d_new_overlap, &t.n_new_bases, t.stats);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_walks_pileup_ex: walks_pileup, and the vote keys of the batch's insertions of S2K_LONG_INS_MIN .. S2K_LONG_INS_MAX bases written
    // compact to d_long_keys (capacity in keys; nullptr: none).  n_candidates bounds the keys and is set on S2K_ERR_CAPACITY too, which
    // throws (nothing written, the pile included): size the buffer by a count of such I runs over al.ops, or retry with n_candidates.
    struct PileupKeys {
        PileupStats stats;
        uint64_t n_candidates, n_long_keys;
    };
    PileupKeys walks_pileup_ex(const s2k_walk_out &walks, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off, const uint8_t *d_out,
                               uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, const Pool &query, const s2k_align_out &al, const s2k_pile &pile,
                               uint64_t *d_long_keys, uint64_t capacity, uint32_t max_shift = S2K_PILEUP_MAX_SHIFT, uint64_t *n_candidates = nullptr) {
        PileupKeys t{};
        s2k_status st = s2k_walks_pileup_ex(ctx_, walks.capacity, walks.first_step, walks.n_steps, walks.path_start, walks.path_end, walks.flags, d_step_unitig,
                                            n_steps, d_out_off, d_out, n_bases, d_overlap, n_unitigs, query.bytes, query.n_bytes, query.begin, al.flags,
                                            al.ops_off, al.n_ops, al.ops, al.capacity, max_shift, &pile, t.stats.v, d_long_keys, capacity, &t.n_candidates,
                                            &t.n_long_keys);
        if (n_candidates) *n_candidates = t.n_candidates;
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_pileup_consensus_ex: pileup_consensus with the counted vote keys (ascending, as s2k_counter_finish writes them); stats[5] and
    // stats[6] are the positions and the bases of the long insertions called.  n_long_keys 0: pileup_consensus.
    Consensus pileup_consensus_ex(const s2k_pile &pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap,
                                  uint64_t n_unitigs, uint32_t min_cov, const uint64_t *d_long_keys, const uint32_t *d_long_counts, uint64_t n_long_keys,
                                  uint64_t *d_new_out_off = nullptr, uint8_t *d_new_out = nullptr, uint64_t capacity = 0, uint64_t *d_pos_map = nullptr,
                                  uint32_t *d_new_overlap = nullptr) {
        Consensus t{};
        s2k_status st = s2k_pileup_consensus_ex(ctx_, &pile, d_out_off, d_out, n_bases, d_overlap, n_unitigs, min_cov, d_new_out_off, d_new_out, capacity,
                                                d_pos_map, d_new_overlap, &t.n_new_bases, t.stats, d_long_keys, d_long_counts, n_long_keys);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_walks_segments: every walk cut into segment pairs at a thinned, strictly increasing subset of its anchor k-min-mers (`walks`:
    // the records s2k_paths_walks wrote, walk_off included; `paths`: unitig, pos, count of the steps they were made on; `lift`: the
    // decomposition and its base coordinates as paths_walks takes them; d_q_begin, d_tgt_off, d_bad per walk; `source`: the paths
    // s2k_table_thread wrote for the same reads, where every step of them went (nullptr: the identity / src->pos) and the batch's
    // extraction).  out nullptr: the sizes only.  Returns the segments and the S2K_SEGMENT_STATS counters; throws on S2K_ERR_CAPACITY
    // too (nothing written).
    struct SegmentLift {
        const uint64_t *uni_off;
        const uint32_t *members;
        const uint8_t *circular;
        uint64_t n_unitigs;
        const uint64_t *member_off, *out_off;
        const uint32_t *overlap, *seq_len;
        uint64_t n_nodes;
    };
    struct SegmentSource {
        const s2k_thread_out *paths;
        uint64_t n_steps;
        const uint64_t *step; // per source step, S2K_NO_STEP for none
        const uint32_t *pos;
        const s2k_device_out *in;
    };
    struct Segments {
        uint64_t n_segments;
        uint64_t stats[S2K_SEGMENT_STATS];
    };
    Segments walks_segments(uint64_t n_reads, const s2k_walk_out &walks, uint64_t n_walks, const s2k_thread_out &paths, uint64_t n_steps,
                            const SegmentLift &lift, const uint64_t *d_q_begin, const uint64_t *d_tgt_off, const uint8_t *d_bad, const SegmentSource &source,
                            uint32_t seg_len = S2K_SEGMENT_LEN, const s2k_segment_out *out = nullptr) {
        Segments t{};
        s2k_status st = s2k_walks_segments(ctx_, n_reads, &walks, n_walks, &paths, n_steps, lift.uni_off, lift.members, lift.circular, lift.n_unitigs,
                                           lift.member_off, lift.out_off, lift.overlap, lift.seq_len, lift.n_nodes, d_q_begin, d_tgt_off, d_bad, source.paths,
                                           source.n_steps, source.step, source.pos, source.in, seg_len, out, &t.n_segments, t.stats);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return t;
    }
    // s2k_align_join: the alignments align_pairs wrote for the segment pairs (`seg`, seg.capacity = the runs seg.ops holds) joined into
    // one alignment per walk.  out nullptr: the size only.  Returns the joined runs; throws on S2K_ERR_CAPACITY too (nothing written).
    uint64_t align_join(uint64_t n_walks, const uint64_t *d_seg_off, const uint8_t *d_bad, uint64_t n_segments, const s2k_align_out &seg,
                        const s2k_align_out *out = nullptr) {
        uint64_t n_ops_total = 0;
        s2k_status st = s2k_align_join(ctx_, n_walks, d_seg_off, d_bad, n_segments, &seg, out, &n_ops_total);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_ops_total;
    }
    // s2k_walks_gaf: the GAF lines of the walks (`walks`: walk_off and the record arrays s2k_paths_walks wrote) as bytes on the device.
    // names.bytes / names.off nullptr: the decimal first_read + r; d_read_len nullptr: *; al nullptr: no alignment columns (al->capacity
    // = the runs al->ops holds).  d_text nullptr: the sizes only.  Returns the bytes of all lines; throws on S2K_ERR_CAPACITY too
    // (nothing written).
    struct Names {
        const uint8_t *bytes;
        const uint64_t *off; // n_reads + 1
        uint64_t n_bytes;
    };
    uint64_t walks_gaf(uint64_t n_reads, const s2k_walk_out &walks, uint64_t n_walks, const uint32_t *d_step_unitig, uint64_t n_steps, const Names &names = {},
                       uint64_t first_read = 0, const uint64_t *d_read_len = nullptr, const s2k_align_out *al = nullptr, uint8_t *d_text = nullptr,
                       uint64_t capacity = 0, uint64_t *d_line_off = nullptr) {
        uint64_t n_bytes = 0;
        s2k_status st = s2k_walks_gaf(ctx_, n_reads, &walks, n_walks, d_step_unitig, n_steps, names.bytes, names.off, names.n_bytes, first_read, d_read_len, al,
                                      d_text, capacity, d_line_off, &n_bytes);
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(ctx_));
        return n_bytes;
    }
    s2k_ctx *raw() { return ctx_; }

  private:
    s2k_ctx *ctx_;
};

// Accumulating k-min-mer count (s2k_counter_*) over batches and files: add() device-resident hashes batch by batch, finish() the
// solid pairs in ascending key order (d_keys / d_counts may be nullptr: sizes only).  Destroy it before its Engine.
class Counter {
  public:
    explicit Counter(Engine &eng) : eng_(&eng) {
        s2k_status st;
        c_ = s2k_counter_create(eng.raw(), &st);
        if (!c_) throw Error(st, std::string("s2k_counter_create: ") + s2k_strerror(st));
    }
    Counter(const Counter &) = delete;
    Counter &operator=(const Counter &) = delete;
    ~Counter() { s2k_counter_destroy(c_); }
    void add(const uint64_t *d_hash, uint64_t n) { check(s2k_counter_add(c_, d_hash, n)); }
    Engine::CountSizes finish(uint32_t min_count, uint64_t *d_keys = nullptr, uint32_t *d_counts = nullptr, uint64_t capacity = 0) {
        Engine::CountSizes r{0, 0};
        check(s2k_counter_finish(c_, min_count, d_keys, d_counts, capacity, &r.n_distinct, &r.n_kept));
        return r;
    }
    s2k_counter *raw() { return c_; }

  private:
    void check(s2k_status st) {
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(eng_->raw()));
    }
    Engine *eng_;
    s2k_counter *c_;
};

// Look-ups against a count table (s2k_table_*): the table borrows d_keys / d_counts (d_counts may be nullptr: membership), which must
// stay valid and unchanged while it lives.  lookup() writes each query's count (0 if absent); filter() keeps each read's k-min-mers
// whose count is at least min_count and returns how many were kept (throws on S2K_ERR_CAPACITY too); edges() writes the graph edge
// keys of the reads (s2k_table_edges; d_edge_keys nullptr: size only) and returns how many there are (throws on S2K_ERR_CAPACITY too).
// Destroy it before its Engine.
class Table {
  public:
    Table(Engine &eng, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n) : eng_(&eng) {
        s2k_status st;
        t_ = s2k_table_create(eng.raw(), d_keys, d_counts, n, &st);
        if (!t_) throw Error(st, std::string("s2k_table_create: ") + s2k_strerror(st) + ": " + s2k_last_error(eng.raw()));
    }
    Table(const Table &) = delete;
    Table &operator=(const Table &) = delete;
    ~Table() { s2k_table_destroy(t_); }
    void lookup(const uint64_t *d_query, uint64_t n, uint32_t *d_out) { check(s2k_table_lookup(t_, d_query, n, d_out)); }
    uint64_t filter(uint64_t n_reads, const s2k_device_out &in, uint32_t min_count, const s2k_solid_out &out) {
        uint64_t n_kept = 0;
        check(s2k_table_filter(t_, n_reads, &in, min_count, &out, &n_kept));
        return n_kept;
    }
    uint64_t edges(uint64_t n_reads, const s2k_device_out &in, uint32_t min_count, uint64_t *d_edge_keys = nullptr, uint64_t capacity = 0) {
        uint64_t n_edges = 0;
        check(s2k_table_edges(t_, n_reads, &in, min_count, d_edge_keys, capacity, &n_edges));
        return n_edges;
    }
    // s2k_table_representatives: d_rep[i] = min(d_rep[i], ordinal_base + x) over the batch's items x whose hash is key i (d_rep: one
    // uint64_t per key, 0xFF bytes before the first batch)
    void representatives(uint64_t n_reads, const s2k_device_out &in, uint64_t ordinal_base, uint64_t *d_rep) {
        check(s2k_table_representatives(t_, n_reads, &in, ordinal_base, d_rep));
    }
    // s2k_table_node_sequences: the records and bytes of the nodes whose representative lies in this batch (`in` written with
    // S2K_FLAG_WANT_MINIMIZERS); nodes nullptr: the size only.  Returns the bytes the batch adds to the pool (throws on
    // S2K_ERR_CAPACITY too).
    uint64_t node_sequences(uint64_t n_reads, const s2k_device_out &in, uint32_t k, const uint8_t *d_bases, const uint64_t *d_read_off,
                            uint64_t ordinal_base, const uint64_t *d_rep, const s2k_node_seqs *nodes = nullptr, uint64_t pool_used = 0) {
        uint64_t n_bytes = 0;
        check(s2k_table_node_sequences(t_, n_reads, &in, k, d_bases, d_read_off, ordinal_base, d_rep, nodes, pool_used, &n_bytes));
        return n_bytes;
    }
    // s2k_table_vote_keys: the three vote keys (whole, forward end, reverse end) of every item of the batch whose hash is in the table,
    // in item order, for a Counter; d_keys nullptr: the size only.  Returns the number of keys (throws on S2K_ERR_CAPACITY too).
    uint64_t vote_keys(uint64_t n_reads, const s2k_device_out &in, uint32_t k, const uint8_t *d_bases, const uint64_t *d_read_off,
                       uint64_t *d_keys = nullptr, uint64_t capacity = 0) {
        uint64_t n_keys = 0;
        check(s2k_table_vote_keys(t_, n_reads, &in, k, d_bases, d_read_off, d_keys, capacity, &n_keys));
        return n_keys;
    }
    // s2k_table_vote_representatives: d_best[i] = max(d_best[i], votes and ordinal of item x) over the batch's items x whose hash is
    // key i, the votes from `votes`, the table over the counted vote keys of every batch (d_best: one uint64_t per key, zeroed before
    // the first batch; Engine::vote_ordinals turns it into the d_rep of node_sequences)
    void vote_representatives(Table &votes, uint64_t n_reads, const s2k_device_out &in, uint32_t k, const uint8_t *d_bases,
                              const uint64_t *d_read_off, uint64_t ordinal_base, uint64_t *d_best) {
        check(s2k_table_vote_representatives(t_, votes.t_, n_reads, &in, k, d_bases, d_read_off, ordinal_base, d_best));
    }
    // s2k_table_thread: each read's path through the unitigs whose node places are d_place (Engine::unitig_node_places; n_nodes = the
    // table's keys): out.path_off always, the step arrays of `out` when they fit (all nullptr: the sizes only); d_uni_items (may be
    // nullptr, one uint64_t per unitig) gains every step's count.  Returns the number of steps (throws on S2K_ERR_CAPACITY too).
    uint64_t thread(uint64_t n_reads, const s2k_device_out &in, uint32_t min_count, const s2k_node_place *d_place, uint64_t n_nodes,
                    const s2k_thread_out &out, uint64_t n_unitigs, uint64_t *d_uni_items = nullptr) {
        uint64_t n_steps = 0;
        check(s2k_table_thread(t_, n_reads, &in, min_count, d_place, n_nodes, &out, d_uni_items, n_unitigs, &n_steps));
        return n_steps;
    }
    s2k_table *raw() { return t_; }

  private:
    void check(s2k_status st) {
        if (st != S2K_OK) throw Error(st, std::string(s2k_strerror(st)) + ": " + s2k_last_error(eng_->raw()));
    }
    Engine *eng_;
    s2k_table *t_;
};

class KminmersIterator { // src/lib.rs:70-131: per-read facade
  public:
    KminmersIterator(Engine &eng, std::string_view seq, size_t l, size_t k, double density, HashMode mode)
        : batch_(eng.extract(std::vector<std::string_view>{seq}, l, k, density, mode)) {}
    struct iterator {
        const Batch *b;
        uint64_t i;
        KminmerHash operator*() const { return b->item(0, i); }
        iterator &operator++() {
            ++i;
            return *this;
        }
        bool operator!=(const iterator &o) const { return i != o.i; }
    };
    iterator begin() const { return iterator{&batch_, 0}; }
    iterator end() const { return iterator{&batch_, batch_.n_kminmers()}; }
    size_t size() const { return (size_t)batch_.n_kminmers(); }

  private:
    Batch batch_;
};

// The crate's minimizer iterators (re-exported at src/lib.rs:6-13), over S2K_FLAG_WANT_MINIMIZERS.  Like the reference they take
// the u32 hash bound, not a density.  One GPU call per sequence: for throughput use Engine::extract with the flag on a batch.
// l > seq.size() throws as KSizeOutOfRange does (src/nthash_hpc.rs:117-121); seq.size() == l is accepted as in the reference.
struct Minimizer { // NtHashHPCIterator::Item = (start, end, hash), src/nthash_hpc.rs:193
    size_t start, end;
    uint32_t hash;
};
template <HashMode MODE>
class MinimizerIterator {
  public:
    MinimizerIterator(Engine &eng, std::string_view seq, size_t l, uint32_t hash_bound) {
        if (l > seq.size()) throw Error(S2K_ERR_L_RANGE, "K size is out of range for the given sequence size"); // src/nthash_hpc.rs:19-22
        if (seq.size() == l) {
            // Accepted by the reference's iterators (only l > len is KSizeOutOfRange).  The scalar Hpc iterator yields nothing then (its only
            // l-mer is the last one, src/nthash_hpc.rs:265-267); the SIMD ones may yield the single l-mer.  The kernels follow
            // KminmersIterator (len <= l: nothing, src/lib.rs:97), so that l-mer is computed on the GPU on the sequence plus one base
            // that starts a new run, and only what lies inside the original sequence is kept (end_).
            if (MODE == HashMode::Hpc) return; // empty batch
            std::string ext(seq);
            ext.push_back(seq.back() == 'A' ? 'C' : 'A');
            batch_ = eng.extract(std::vector<std::string_view>{ext}, l, 1, s2k_density_for_bound(hash_bound), MODE, S2K_FLAG_WANT_MINIMIZERS);
            const s2k_result &r = batch_.raw();
            end_ = (r.n_minimizers >= 1 && r.mn_j[0] == 0 && r.mn_jend[0] < l) ? 1 : 0;
            limited_ = true;
            return;
        }
        batch_ = eng.extract(std::vector<std::string_view>{seq}, l, 1, s2k_density_for_bound(hash_bound), MODE, S2K_FLAG_WANT_MINIMIZERS);
    }
    struct iterator {
        const s2k_result *r;
        uint64_t i;
        Minimizer operator*() const { return Minimizer{r->mn_j[i], r->mn_jend[i], r->mn_hash[i]}; }
        iterator &operator++() {
            ++i;
            return *this;
        }
        bool operator!=(const iterator &o) const { return i != o.i; }
    };
    iterator begin() const { return iterator{&batch_.raw(), 0}; }
    iterator end() const { return iterator{&batch_.raw(), size()}; }
    size_t size() const { return limited_ ? (size_t)end_ : (size_t)batch_.n_minimizers(); }

  private:
    Batch batch_;
    uint64_t end_ = 0;     // seq.size() == l: how many of the batch's minimizers lie inside the original sequence (0 or 1)
    bool limited_ = false;
};
using NtHashHPCIterator = MinimizerIterator<HashMode::Hpc>;         // src/nthash_hpc.rs:99-283: `<=`, last HPC l-mer dropped, end = last base of the last run
using NtHashHPCSIMDIterator = MinimizerIterator<HashMode::HpcSimd>; // src/nthash_hpc_simd.rs:17-68: `<` vs f32 bound, end = start of the last run
using NtHashSIMDIterator = MinimizerIterator<HashMode::Simd>;       // src/nthash_avx512_32.rs:14-164: Item = (pos, hash): use .start and .hash

inline uint32_t hash_bound(double density) { return s2k_hash_bound(density); } // src/lib.rs:91

} // namespace s2k
