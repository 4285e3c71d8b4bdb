/*
 * s2k.h -- C ABI of the MI355X-native k-min-mer extraction engine.
 *
 * This is the drop-in boundary for ONE path of rchikhi/rust-seq2kminmers: "reads in -> ordered
 * stream of k-min-mers out".  In the reference that path is
 *     KminmersIterator::new(seq, l, k, density, mode)      src/lib.rs:89-131
 *     impl Iterator for KminmersIterator { Item = KminmerHash }   src/lib.rs:179-270
 *     struct KminmerHash { hash, start, end, offset, rev }  src/kminmer.rs:128-135
 * called once per read from a thread pool (src/main.rs:65-79).  A GPU needs >= 10^4 reads per
 * launch, so the ABI is batch-oriented: n_reads reads stored back to back, one call, SoA results;
 * the per-read Iterator shape is rebuilt on top of it by include/s2k.hpp (C++) and by the Rust shim
 * shown in INTEGRATION.md.  The crate's own precedent for an opaque-handle C ABI is
 * src/nthash_c.rs:14-29 (create / roll / get / destroy).
 *
 * Conventions: plain C types only; the caller owns inputs; the library owns s2k_result buffers until
 * s2k_result_free(); nothing panics or throws across the ABI -- parameter violations that make the
 * reference panic (src/lib.rs:99 unwrap of KSizeTooBig, src/nthash_hpc.rs:133 assert!(k<256),
 * src/lib.rs:246 underflow at k==0) come back as status codes.  One s2k_ctx per (thread, device);
 * contexts are independent.  All results are bit-exact to the reference's scalar path
 * (HashMode::Regular / HashMode::Hpc); the Simd / HpcSimd *result semantics* (strict '<', f32 bound,
 * start-of-run end, kept last l-mer, low-nibble seed map -- SURVEY.md 8a traps i-vi) are selectable.
 */
#ifndef S2K_H
#define S2K_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI history.  1: round-1 surface.  2: + s2k_set_host_batch, s2k_hpc_device_ex, s2k_count_device, s2k_partition_device,
 * S2K_FLAG_NO_PACK2; s2k_extract sends 2-bit packed bases and pipelines sub-batches by default; the arrays of an s2k_result
 * are NULL when their count is 0; device-resident read tables are validated on the device (S2K_ERR_INVALID_ARG /
 * S2K_ERR_READ_TOO_LONG from s2k_extract_device, s2k_sync and s2k_hpc_device*); S2K_ERR_NON_ASCII is no longer returned;
 * + s2k_trim, s2k_density_for_bound, S2K_FLAG_LEGACY_PATH; s2k_counts.path tells the descriptor path (0) from the legacy one (2).
 * (Round 4 only ADDED entry points -- the benchmark helpers s2k_synth_hifi_lengths / s2k_synth_hifi_device, and s2k_chain_after: no existing entry point or
 * struct changed, the version stays 2.)
 * (s2k_count_device_ex and S2K_COUNT_SORTED were added later the same way: an added entry point, the version stays 2.)
 * (s2k_count_merge_device, the opaque s2k_counter with s2k_counter_create / _destroy / _add / _finish, and s2k_run_file_count were
 * added the same way: added entry points and one opaque type, the version stays 2.)
 * (The opaque s2k_table with s2k_table_create / _destroy / _lookup / _filter and the struct s2k_solid_out were added the same way:
 * added entry points, one opaque type and one new struct; no existing entry point or struct changed, the version stays 2.)
 * (s2k_table_edges and s2k_graph_adjacency were added the same way: added entry points, the version stays 2.)
 * (s2k_graph_unitigs, s2k_graph_unitig_edges, s2k_graph_unitigs_last_steps and the struct s2k_unitig_out were added the same way:
 * added entry points and one new struct, the version stays 2.)
 * (s2k_table_representatives, s2k_table_node_sequences, s2k_unitig_sequences and the struct s2k_node_seqs were added the same way.)
 * (s2k_paths_spans and s2k_graph_resolve_mask were added the same way: added entry points, the version stays 2.)
 * (s2k_paths_bridge was added the same way: an added entry point, the version stays 2.)
 * (s2k_unitig_copy_places, s2k_paths_lift and S2K_NO_COPY were added the same way: added entry points, the version stays 2.)
 * A binding must refuse a library whose s2k_abi_version() differs from the header it was built against. */
#define S2K_ABI_VERSION 2

typedef struct s2k_ctx s2k_ctx; /* opaque; cf. nthashc_create/destroy, src/nthash_c.rs:14-29 */

typedef enum s2k_status {
    S2K_OK = 0,
    S2K_ERR_INVALID_ARG = 1,   /* NULL pointer, unknown mode, a read table that does not start at 0 / is not non-decreasing / does not end at n_bases */
    S2K_ERR_L_RANGE = 2,       /* l == 0 or l >= 256 (src/nthash_hpc.rs:123-125,133); Simd modes: l > 31 (src/nthash_avx512_32.rs:33) */
    S2K_ERR_K_RANGE = 3,       /* k == 0 (src/lib.rs:246 would underflow) or k > 4096 */
    S2K_ERR_READ_TOO_LONG = 4, /* a read longer than 2^32-2 bases (positions are u32, cf. src/nthash_hpc_simd.rs:26) */
    S2K_ERR_DEVICE = 5,        /* HIP runtime error; s2k_last_error() has the text */
    S2K_ERR_NOMEM = 6,
    S2K_ERR_CAPACITY = 7,      /* caller-provided device output too small; counts say what is needed */
    S2K_ERR_NO_DEVICE = 8,     /* no gfx950 device visible: there is NO CPU fallback */
    S2K_ERR_NON_ASCII = 9      /* reserved: returned by ABI 1 for bytes >= 0x80 in Hpc mode; every byte value is accepted now */
} s2k_status;

/* HashMode, src/lib.rs:21-27 */
typedef enum s2k_mode {
    S2K_MODE_REGULAR = 0, /* src/lib.rs:215-230 */
    S2K_MODE_HPC = 1,     /* NtHashHPCIterator, src/nthash_hpc.rs:115-283 */
    S2K_MODE_SIMD = 2,    /* result semantics of NtHashSIMDIterator, src/nthash_avx512_32.rs:32-164 */
    S2K_MODE_HPCSIMD = 3  /* result semantics of NtHashHPCSIMDIterator, src/nthash_hpc_simd.rs:35-68 */
} s2k_mode;

enum {
    S2K_FLAG_WANT_MINIMIZERS = 1u << 0, /* also return the (j, jend, hash32) triples (NtHashHPCIterator::Item, src/nthash_hpc.rs:193) */
    S2K_FLAG_FORCE_SERIAL = 1u << 1,    /* use the read-serial kernels (exact for every input; slow) instead of the tiled ones */
    S2K_FLAG_NO_PACK2 = 1u << 2,        /* s2k_extract, s2k_run_file: send the text as it is instead of 2-bit packed (+ exception list) over PCIe */
    S2K_FLAG_LEGACY_PATH = 1u << 3      /* tiled kernels with the round-2 records (16 B with the read index, per-read scans; counts.path 2) instead of the descriptor path */
};

typedef struct s2k_params {
    uint32_t l;       /* minimizer length            (src/lib.rs:89 `l`) */
    uint32_t k;       /* k-min-mer order             (src/lib.rs:89 `k`) */
    double density;   /* FH = f64                    (src/lib.rs:34,89) */
    int32_t mode;     /* s2k_mode */
    uint32_t flags;
} s2k_params;

typedef struct s2k_counts {
    uint64_t n_reads;
    uint64_t n_bases;
    uint64_t n_minimizers;
    uint64_t n_kminmers;
    uint64_t xor_hash;   /* XOR of all k-min-mer hashes (cheap whole-run checksum) */
    uint32_t hash_bound; /* the u32 bound of src/lib.rs:91 that was used */
    uint32_t path;       /* 0 = tiled kernels, descriptor path (8-byte tile-relative records); 1 = read-serial kernels;
                          * 2 = tiled kernels, legacy records (k > 32, a tile with more than 30 read starts, S2K_FLAG_LEGACY_PATH) */
} s2k_counts;

/* Host-side result, SoA.  Item i of read r (km_off[r] <= i < km_off[r+1]) is
 * KminmerHash{ hash[i], start[i], end[i], offset = i - km_off[r], rev[i] }  (src/kminmer.rs:128-135).
 * hash / start / end / rev are NULL when n_kminmers == 0, the mn_* arrays when n_minimizers == 0. */
typedef struct s2k_result {
    uint64_t n_reads;
    uint64_t n_kminmers;
    uint64_t *km_off; /* n_reads + 1 */
    uint64_t *hash;   /* KH = u64, src/lib.rs:37 */
    uint32_t *start;
    uint32_t *end;
    uint8_t *rev;
    /* only with S2K_FLAG_WANT_MINIMIZERS, else NULL / 0 */
    uint64_t n_minimizers;
    uint64_t *mn_off; /* n_reads + 1 */
    uint32_t *mn_j;
    uint32_t *mn_jend;
    uint32_t *mn_hash; /* H = u32, src/lib.rs:31 */
    s2k_counts counts;
    void *_owner;
} s2k_result;

/* Device-resident output buffers provided by the caller (device pointers, capacities in items). */
typedef struct s2k_device_out {
    uint64_t km_capacity;
    uint64_t *km_off; /* n_reads + 1, required */
    uint64_t *hash;   /* may be NULL to skip */
    uint32_t *start;
    uint32_t *end;
    uint8_t *rev;
    uint64_t mn_capacity; /* 0 => minimizer triples not wanted */
    uint64_t *mn_off;
    uint32_t *mn_j;
    uint32_t *mn_jend;
    uint32_t *mn_hash;
} s2k_device_out;

/* ---- lifecycle ------------------------------------------------------------------------------- */
int s2k_abi_version(void);
int s2k_device_count(void);
/* Creates a context on HIP device `device`.  Fails with S2K_ERR_NO_DEVICE when no GPU is visible. */
s2k_ctx *s2k_create(int device, s2k_status *status);
void s2k_destroy(s2k_ctx *ctx);
/* Use an existing hipStream_t (e.g. torch's current stream) instead of the device's shared k-min-mer stream: the k-min-mer stage, the totals
 * and the counts copy of every call run on it (results are complete in its order), the minimizer kernels on the device's minimizer stream,
 * which waits for this stream at the start of each call. */
s2k_status s2k_set_stream(s2k_ctx *ctx, void *hip_stream);
/* Double buffering with two contexts on one device (a loop over many device-resident batches): the minimizer kernels of every context on a
 * device run in call order on one stream of the library's, and the rest of a call on another (or the caller's), so the tail of a's call (its
 * last k-min-mer kernel, the totals, the host's look at the counts) runs beside the first chunk of b's next one, and two persistent kernels
 * never compete for the device.  s2k_chain_after(b, a) tells b that a call of a's follows each of its own (it sizes its chunks for that).
 * Chain both ways (a after b, b after a) and alternate the calls from ONE host thread.  prev = NULL removes the link;
 * s2k_destroy(prev) removes every link to prev by itself (the survivor then runs unchained), from any thread: links are read and cut under one
 * lock.  A prev that is not a live context is refused (S2K_ERR_INVALID_ARG).  Results do not depend on it. */
s2k_status s2k_chain_after(s2k_ctx *ctx, s2k_ctx *prev);
/* s2k_extract cuts a call into sub-batches of whole reads of about `bases` bases each (default 2^29; 0 restores it) and
 * pipelines them: H2D of one, kernels of the previous, D2H of the one before run side by side.  Results do not depend
 * on it. */
s2k_status s2k_set_host_batch(s2k_ctx *ctx, uint64_t bases);
const char *s2k_strerror(s2k_status st);
const char *s2k_last_error(const s2k_ctx *ctx);

/* (density * u32::MAX as f64) as u32 -- src/lib.rs:91 */
uint32_t s2k_hash_bound(double density);
/* A density d with s2k_hash_bound(d) == bound, for callers that hold the u32 bound itself -- the crate's minimizer iterators
 * take it instead of a density: NtHashHPCIterator::new(seq, k, hash_bound) src/nthash_hpc.rs:115, NtHashSIMDIterator::new
 * src/nthash_avx512_32.rs:32, NtHashHPCSIMDIterator::new src/nthash_hpc_simd.rs:35. */
double s2k_density_for_bound(uint32_t bound);

/* ---- the hot path ---------------------------------------------------------------------------- */
/* Replaces: for each read r { KminmersIterator::new(&bases[read_off[r]..read_off[r+1]], l, k, density,
 * mode)?.collect() } -- src/lib.rs:89,179 driven by src/main.rs:65-79.  Host buffers in, host SoA out
 * (library-owned; release with s2k_result_free).  Reads with len <= l yield nothing (src/lib.rs:97).
 * s2k_result_free hands the arrays back to a pool kept by the context that made them (fresh gigabyte allocations cost
 * more in page faults than the copy): a long-lived context retains the arrays of up to two freed results (18 blocks, sized
 * by the largest recent call) of host memory until s2k_trim() or s2k_destroy(). */
s2k_status s2k_extract(s2k_ctx *ctx, const uint8_t *bases, const uint64_t *read_off, uint64_t n_reads,
                       const s2k_params *params, s2k_result *out);
void s2k_result_free(s2k_result *res);

/* Releases what a context keeps between calls: idle host result blocks and the device workspace (both grow again on
 * demand).  Call it when a long-lived context has seen an unusually large batch. */
s2k_status s2k_trim(s2k_ctx *ctx);

/* Same computation with inputs and outputs resident in HBM: d_read_off[0] must be 0, the table non-decreasing and
 * d_read_off[n_reads] == n_bases (read r = d_bases[d_read_off[r] .. d_read_off[r+1])) -- checked on the device: a table
 * that breaks this yields S2K_ERR_INVALID_ARG (a read longer than 2^32-2 bases S2K_ERR_READ_TOO_LONG) from this call
 * or, with counts == NULL, from s2k_sync(), and nothing is computed.  A d_bases pointer that is not 16-byte aligned is
 * accepted: the stream is first copied to an aligned buffer (one device-to-device pass) and takes the same tiled
 * kernels.  Enqueued on the context's stream; if
 * `counts` is non-NULL the call waits for completion and fills it (and returns S2K_ERR_CAPACITY if
 * an output capacity was too small -- counts then hold the required sizes, xor_hash is still the XOR of ALL k-min-mers,
 * km_off / mn_off are whole, the given arrays hold the first km_capacity / mn_capacity items, and nothing is written past
 * them; the same on the descriptor, legacy and read-serial paths).  With counts == NULL the
 * call returns after enqueueing; s2k_sync() later waits and reports the same status/counts. */
s2k_status s2k_extract_device(s2k_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_read_off,
                              uint64_t n_reads, uint64_t n_bases, const s2k_params *params,
                              const s2k_device_out *out, s2k_counts *counts);
s2k_status s2k_sync(s2k_ctx *ctx, s2k_counts *counts);

/* ---- standalone homopolymer compression (src/hpc.rs:28-41 hpc, :44-147 encode_rle_simd) ---------- */
/* Per read: compressed string + run-start positions (read-relative); same layout rules as s2k_extract_device.
 * d_hpc_off: n_reads+1 prefix of
 * run counts; d_hpc / d_pos (either may be NULL) receive up to `capacity` entries. */
s2k_status s2k_hpc_device(s2k_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                          uint64_t n_bases, uint64_t *d_hpc_off, uint8_t *d_hpc, uint32_t *d_pos,
                          uint64_t capacity, uint64_t *n_runs);
/* Same with flags.  S2K_HPC_RLE_ALPHABET selects the run rule of `encode_rle` (src/hpc.rs:7-25): a repeated character
 * collapses only if it is one of "ACTGactgNn" (src/hpc.rs:14); without it any repeated byte collapses (`hpc`
 * src/hpc.rs:28-41, `encode_rle_simd` src/hpc.rs:44-147).  Not reproduced on the device: the two scalar functions start
 * from prev_char = '#', so they drop '#' characters that are followed by another character, report a stale position for
 * the run after a '#', and return "#" for an empty string; here '#' is an ordinary byte and an empty read has no runs
 * (the host facades add the empty-string case and refuse input that contains '#'). */
#define S2K_HPC_RLE_ALPHABET 1u
s2k_status s2k_hpc_device_ex(s2k_ctx *ctx, const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t n_reads,
                             uint64_t n_bases, uint32_t flags, uint64_t *d_hpc_off, uint8_t *d_hpc, uint32_t *d_pos,
                             uint64_t capacity, uint64_t *n_runs);

/* ---- downstream of the path: k-min-mer counting ------------------------------------ */
/* What the consumer of the iterator does in rust-mdbg (a concurrent map keyed by the k-min-mer hash; the reference only
 * hints at it, src/lib.rs:256-257; KminmerHash is Eq/Hash by `hash` alone, src/kminmer.rs:181-204): the distinct values
 * of d_hash[0..n) and how often each occurs.  d_keys / d_counts (either may be NULL) receive up to `capacity` pairs in
 * unspecified order; *n_distinct is always set (S2K_ERR_CAPACITY when it exceeds capacity). */
s2k_status s2k_count_device(s2k_ctx *ctx, const uint64_t *d_hash, uint64_t n, uint64_t *d_keys, uint32_t *d_counts,
                            uint64_t capacity, uint64_t *n_distinct);
/* Counting with an abundance cutoff (what rust-mdbg keeps: the "solid" k-min-mers): the pairs (key, count) of every distinct value
 * of d_hash[0..n) that occurs at least min_count times (min_count 0 and 1 both mean all).  With S2K_COUNT_SORTED the pairs come in
 * ascending order of key (unsigned 64-bit) and the output is bit-identical from call to call; without it the order is unspecified.
 * *n_distinct (distinct keys before the cutoff) and *n_kept (after it) are always set; S2K_ERR_CAPACITY when *n_kept > capacity and
 * d_keys or d_counts is non-NULL (nothing is written then); both may be NULL (sizes only).  Every 64-bit value is a key, 0 and
 * 2^64-1 included.  n >= 2^32 (counts are uint32_t) and unknown flag bits are refused (S2K_ERR_INVALID_ARG).  Runs on the context's
 * stream, in the context's grow-only workspace (about 20 bytes per key); returns when the pairs are written. */
#define S2K_COUNT_SORTED 1u /* pairs in ascending order of key (unsigned 64-bit) */
s2k_status s2k_count_device_ex(s2k_ctx *ctx, const uint64_t *d_hash, uint64_t n, uint32_t min_count, uint32_t flags,
                               uint64_t *d_keys, uint32_t *d_counts, uint64_t capacity, uint64_t *n_distinct, uint64_t *n_kept);
/* Merge of two count tables: (a_keys, a_counts)[0..n_a) and (b_keys, b_counts)[0..n_b), each strictly ascending by key (unsigned
 * 64-bit; every value is a key, 0 and 2^64-1 included), into the table of their union in ascending key order, a key present in both
 * getting the sum of its counts, saturated at 2^32-1.  Pairs whose merged count is under min_count (0 and 1 both mean all) are
 * dropped.  *n_distinct (union before the cutoff) and *n_kept are always set; outputs may both be NULL (sizes only);
 * S2K_ERR_CAPACITY when *n_kept > capacity and an output is non-NULL (nothing written).  An input that is not strictly ascending
 * -> S2K_ERR_INVALID_ARG, detected on the device, nothing written.  Outputs must not overlap the inputs (S2K_ERR_INVALID_ARG).
 * With n_b == 0 the call is the cutoff filter of one table.  Runs on the context's stream; returns when the pairs are written. */
s2k_status s2k_count_merge_device(s2k_ctx *ctx, const uint64_t *d_a_keys, const uint32_t *d_a_counts, uint64_t n_a,
                                  const uint64_t *d_b_keys, const uint32_t *d_b_counts, uint64_t n_b, uint32_t min_count,
                                  uint64_t *d_keys, uint32_t *d_counts, uint64_t capacity, uint64_t *n_distinct, uint64_t *n_kept);
/* Accumulating k-min-mer count over many batches (and files): s2k_counter_add counts each batch of device-resident hashes as it
 * arrives (s2k_count_device_ex, sorted) and keeps the per-batch tables as a stack of runs in which every run is less than half the
 * size of the one below it (a new run is merged down while it is at least half the size of the run under it), so every key takes
 * part in O(log(total / batch)) merges.  s2k_counter_finish merges the stack into one run, keeps it (add may go on; a second finish
 * is one filter pass), and writes the pairs that occur at least min_count times in ascending key order.  Its output is
 * bit-identical to s2k_count_device_ex(concatenation of everything added, min_count, S2K_COUNT_SORTED) except where counts saturate
 * (2^32-1); sizes-only, capacity and refusal rules are those of s2k_count_device_ex.  d_hash of any length (split internally below
 * 2^32 keys); it may be reused when add returns.  Device memory owned by the counter: about 12 B per key of each run in the stack
 * (at most about twice the distinct keys), 12 B per key of the largest batch (scratch), and one merge target while a merge runs;
 * the context's count workspace grows to that of the largest batch.  An add that fails leaves its batch out.  One thread at a time;
 * destroy the counter before its context. */
typedef struct s2k_counter s2k_counter; /* opaque */
s2k_counter *s2k_counter_create(s2k_ctx *ctx, s2k_status *status);
void s2k_counter_destroy(s2k_counter *c);
s2k_status s2k_counter_add(s2k_counter *c, const uint64_t *d_hash, uint64_t n);
s2k_status s2k_counter_finish(s2k_counter *c, uint32_t min_count, uint64_t *d_keys, uint32_t *d_counts, uint64_t capacity,
                              uint64_t *n_distinct, uint64_t *n_kept);
/* Look-ups against a count table (rust-mdbg's second pass: each read's k-min-mers with their abundance, the solid ones kept).
 * s2k_table_create indexes (d_keys, d_counts)[0..n), any table strictly ascending by key (unsigned 64-bit) -- what
 * s2k_count_device_ex(S2K_COUNT_SORTED), s2k_count_merge_device and s2k_counter_finish write.  The table BORROWS the two arrays: they
 * must stay valid and unchanged until s2k_table_destroy.  d_counts == NULL makes a membership table (every key present counts 1).
 * n == 0 is allowed (every look-up gives 0); n >= 2^32 is refused (S2K_ERR_INVALID_ARG).  Every 64-bit value is a key, 0 and 2^64-1
 * included.  A table that is not strictly ascending is detected on the device: NULL and S2K_ERR_INVALID_ARG.  Device memory owned
 * by the table: a directory over the top B bits of the keys (4 B x (2^B + 1), B chosen for 4-7 keys per bucket, at most 26: at most
 * about 1 B per key, 256 MiB).  Destroy a table before its context; one thread at a time per context, as for every call on it. */
typedef struct s2k_table s2k_table; /* opaque: a read-only index over a count table */
s2k_table *s2k_table_create(s2k_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n, s2k_status *status);
void s2k_table_destroy(s2k_table *t);
/* d_out[i] = the count of d_query[i] in the table, 0 if absent, for i < n (any n, 0 included).  Runs on the context's stream;
 * returns when d_out is written. */
s2k_status s2k_table_lookup(s2k_table *t, const uint64_t *d_query, uint64_t n, uint32_t *d_out);
/* Output of s2k_table_filter (device pointers; capacity in items).  Kept item i of read r (km_off[r] <= i < km_off[r+1]) is
 * KminmerHash{ hash[i], start[i], end[i], offset[i], rev[i] } (src/kminmer.rs:128-135) with offset = its index in the read before
 * filtering (so a consumer can tell which kept k-min-mers were adjacent) and count[i] = the table's count of hash[i]. */
typedef struct s2k_solid_out {
    uint64_t capacity;
    uint64_t *km_off; /* n_reads + 1, required */
    uint64_t *hash;   /* every item array may be NULL */
    uint32_t *start;
    uint32_t *end;
    uint8_t *rev;
    uint32_t *offset;
    uint32_t *count;
} s2k_solid_out;
/* For every read of `in` (the s2k_device_out that s2k_extract_device filled for n_reads reads: km_off and hash required, km_off[0]
 * == 0; start / end / rev optional), the k-min-mers whose count in the table is at least min_count (0 and 1 both mean "present"),
 * in read order.  An output array whose input array is NULL must be NULL (S2K_ERR_INVALID_ARG).  *n_kept is always set and
 * out->km_off always written; the item arrays are written only when *n_kept <= out->capacity, otherwise S2K_ERR_CAPACITY and
 * nothing is written to them; all NULL asks for the sizes only.  Uses the context's grow-only count workspace (shared with
 * s2k_count_device_ex): about 4.2 B per input item.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_table_filter(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t min_count, const s2k_solid_out *out,
                            uint64_t *n_kept);
/* The edges of the minimizer-space de Bruijn graph (rust-mdbg's graph) that the reads of `in` traverse (km_off, hash and rev required,
 * km_off[0] == 0).  Node i is key i of the table (ids are stable while the table lives); the oriented node u = 2 * i + o.  Item j of
 * a read is the oriented node 2 * index(hash[j]) + rev[j]; items j and j + 1 form an adjacency when they belong to the same read and
 * both hashes are in the table with a count of at least min_count (0 and 1 both mean "present"): a non-solid item between two solid
 * ones breaks the chain.  An adjacency gives the edge e = (u, v), key(e) = u << 32 | v, and its twin (v ^ 1, u ^ 1), the same
 * adjacency read on the other strand; it emits key(e) and then key(twin(e)) unless twin(e) == e (a hairpin, v == u ^ 1: one key).
 * A loop u -> u has a distinct twin.  Keys come in item order, bit-identical from call to call.  Counting them
 * (s2k_count_device_ex, an s2k_counter over batches) gives the edge multiplicities, count(e) == count(twin(e)).  *n_edges is always
 * set; the keys are written only when *n_edges <= capacity, otherwise S2K_ERR_CAPACITY and nothing is written; d_edge_keys NULL asks
 * for the size only.  A table of 2^31 keys or more is refused (S2K_ERR_INVALID_ARG: oriented ids are 32-bit).  Uses the context's
 * grow-only count workspace (shared with s2k_count_device_ex): about 4.2 B per input item.  Runs on the context's stream; returns
 * when the keys are written. */
s2k_status s2k_table_edges(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t min_count, uint64_t *d_edge_keys,
                           uint64_t capacity, uint64_t *n_edges);
/* The adjacency (CSR) of a graph over the 2 * n_nodes oriented nodes from its edge keys d_edge_keys[0..n_edges), strictly ascending
 * (unsigned 64-bit, what s2k_count_device_ex(S2K_COUNT_SORTED) and s2k_counter_finish write) with both node ids u = key >> 32 and
 * v = key & 0xFFFFFFFF below 2 * n_nodes.  d_row_off[u] (2 * n_nodes + 1 entries) = the first edge index whose source is >= u, so
 * row_off[2 * n_nodes] == n_edges and the out-edges of u are [row_off[u], row_off[u + 1]); d_dst[i] = the low 32 bits of key i (may
 * be NULL).  An input that breaks the rules is detected on the device: S2K_ERR_INVALID_ARG and nothing written.  Symmetry (every
 * edge's twin present) is not checked.  n_nodes >= 2^31 is refused (S2K_ERR_INVALID_ARG).  Runs on the context's stream; returns when
 * the arrays are written. */
s2k_status s2k_graph_adjacency(s2k_ctx *ctx, const uint64_t *d_edge_keys, uint64_t n_edges, uint64_t n_nodes, uint64_t *d_row_off,
                               uint32_t *d_dst);
/* ---- unitigs: the non-branching paths of the graph compacted ----------------------------------------------
 * Input of both calls: the CSR that s2k_graph_adjacency writes, d_row_off (2 * n_nodes + 1) and d_dst (n_edges; may be NULL when
 * n_edges == 0).  Oriented node u = 2 i + o, twin(u) = u ^ 1, twin of the edge (u, v) = (v ^ 1, u ^ 1), out(u) = row_off[u + 1] -
 * row_off[u].
 * Accepted input: row_off[0] == 0, non-decreasing, row_off[2 n_nodes] == n_edges; every row strictly ascending with ids below
 * 2 n_nodes; and twin-symmetric: for every edge (u, v) the row of v ^ 1 holds u ^ 1 (so in-degree(v) == out(v ^ 1) and no reverse
 * graph is needed).  All of it is checked on the device before anything is written: a violation is S2K_ERR_INVALID_ARG.
 * n_nodes >= 2^31 is refused.
 * Link: next(u) = v iff out(u) == 1, v is that destination, out(v ^ 1) == 1, v != u (a loop) and v != u ^ 1 (a hairpin).  The rule
 * is its own twin (next(u) = v <=> next(v ^ 1) = u ^ 1) and next is injective, so the oriented nodes fall into disjoint chains and
 * cycles, each with a distinct twin that visits the twins in reverse order; none holds both u and u ^ 1.
 * Unitig: one per twin pair of chains / cycles; every node belongs to exactly one, in one orientation.  Of a chain with head h and
 * tail t the kept strand is the one with h < (t ^ 1) (a node without links: 2 i).  Of a cycle the kept strand is the one that holds
 * the smallest oriented id of the two, and it starts there; circular[t] = 1.  Unitigs are numbered by ascending first member of the
 * kept strand, so the outputs are a function of the input alone, bit-identical from call to call.  Oriented unitig U = 2 t + s: s = 0
 * the kept strand, s = 1 its twin (members reversed, each ^ 1). */
typedef struct s2k_unitig_out { /* all device pointers; any may be NULL */
    uint64_t capacity;          /* unitigs that uni_off / circular can hold (uni_off has capacity + 1 entries) */
    uint64_t *uni_off;          /* members of unitig t: [uni_off[t], uni_off[t + 1]); uni_off[n_unitigs] == n_nodes */
    uint32_t *members;          /* n_nodes oriented node ids: the kept strands, in path order */
    uint32_t *node_unitig;      /* n_nodes: the unitig of node i ... */
    uint32_t *node_pos;         /* ... and its position on the kept strand */
    uint8_t *circular;          /* per unitig */
} s2k_unitig_out;
/* *n_unitigs and *n_links (oriented nodes with a next: a link and its twin both count) are always set; the arrays are written only
 * when *n_unitigs <= out->capacity, otherwise S2K_ERR_CAPACITY and nothing is written; out == NULL or all arrays NULL asks for the
 * sizes only.  n_nodes == 0 and n_edges == 0 are valid (n isolated nodes are n unitigs of length 1).  A row of high degree is slow
 * (one lane walks it), never wrong.  Uses the context's grow-only count workspace (shared with s2k_count_device_ex): 60 B per node.
 * Runs on the context's stream; returns when the arrays are written. */
s2k_status s2k_graph_unitigs(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_nodes,
                             const s2k_unitig_out *out, uint64_t *n_unitigs, uint64_t *n_links);
/* The graph between the oriented unitigs: every edge (u, v) of the CSR that is not a link leaves the last member of an oriented
 * unitig U and enters the first member of an oriented unitig V, and gives the key U << 32 | V (a loop on a unitig of length 1 gives
 * U -> U, a hairpin U -> U ^ 1; the closing link of a cycle is a link and gives none), so *n_out == n_edges - n_links.  Keys are
 * written strictly ascending -- s2k_graph_adjacency(d_keys, *n_out, n_unitigs) accepts them as they are, and its result is again
 * twin-symmetric -- and d_src_edge[j] (may be NULL) = the index of the CSR edge key j came from.  d_uni_off, d_members,
 * d_node_unitig and d_node_pos are what s2k_graph_unitigs wrote for the same CSR; neither they nor the CSR are validated again.
 * *n_out is always set; the arrays are written only when *n_out <= capacity, otherwise S2K_ERR_CAPACITY and nothing is written;
 * d_keys NULL asks for the size only.  Workspace: 12 B per oriented unitig. */
s2k_status s2k_graph_unitig_edges(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_nodes,
                                  const uint64_t *d_uni_off, const uint32_t *d_members, const uint32_t *d_node_unitig,
                                  const uint32_t *d_node_pos, uint64_t n_unitigs, uint64_t *d_keys, uint64_t *d_src_edge,
                                  uint64_t capacity, uint64_t *n_out);
/* Measurement helper (tools/unitig_rate.py): host-clock ms of the steps of the last s2k_graph_unitigs call of this process, each
 * of which ends in a host wait -- ms[0] check, ms[1] links + list ranking, ms[2] numbering, ms[3] lengths + scatter -- and the number
 * of jump rounds it ran (ranking, and for cycles the minimum rounds and the second ranking).  Not for concurrent callers. */
void s2k_graph_unitigs_last_steps(double *ms, uint32_t *rounds);
/* ---- simplification: tips clipped and simple bubbles popped on the unitig graph ---------------------------------
 * Input: the compacted graph -- the CSR over the 2 T oriented unitigs (d_row_off, d_dst: what s2k_graph_adjacency writes from the
 * keys of s2k_graph_unitig_edges; twin-symmetric), and per unitig t len[t] = uni_off[t + 1] - uni_off[t] (members) and cnt[t] (the
 * summed counts of its nodes, uint64_t).  For an oriented unitig U = 2 t + s: succ(U) = its CSR row, out(U) = |succ(U)|, pred(U) =
 * { X ^ 1 : X in succ(U ^ 1) }, in(U) = out(U ^ 1).  "The unitig of U" is U >> 1.
 * Order "W beats U" (strict and total over distinct unitigs), decided by the first of these that differs: the higher mean count,
 * cnt[W] * len[U] > cnt[U] * len[W], compared exactly as 128-bit products (no floating point); then more members; then the smaller
 * unitig index.
 * Tip: U is a tip candidate iff out(U) == 0, in(U) >= 1 and len[U] <= max_tip.  U is a removable tip iff it is a candidate and, for
 * every P in pred(U): P is not of U's own unitig, and succ(P) holds some W of another unitig than U that is not a tip candidate or
 * that beats U.  So the best branch at every junction stays, a tip that is some predecessor's only continuation stays, and an
 * isolated unitig (in == out == 0) is no tip.
 * Simple bubble: U is a removable bubble branch iff out(U) == in(U) == 1, len[U] <= max_bubble, its one predecessor P and its one
 * successor S are both of other unitigs than U, and succ(P) holds a W of another unitig than U with out(W) == in(W) == 1, succ(W) ==
 * { S } and W beats U.
 * Removal: unitig t is removed iff 2 t or 2 t + 1 meets either rule; node i is removed iff its unitig is.  Both rules read the same
 * input graph, so the result does not depend on an evaluation order.  max_tip == 0 / max_bubble == 0 switches that rule off (every
 * unitig holds a member).
 * Invariant: a kept oriented unitig with out >= 1 still has a kept successor, so one round creates no new dead end.  (The maximum
 * under "beats" among the candidates of a junction is removable only beside a sibling that is no candidate; a class of parallel
 * bubble branches keeps its maximum, which has out == 1 and so is no tip candidate.)
 *
 * s2k_graph_simplify_mask: d_remove[t] (one byte per unitig, 0 / 1; NULL: the totals only), *n_tips and *n_bubbles = the unitigs
 * removed by each rule (one that meets both counts in both), *n_removed = the bytes set.  One lane per oriented unitig; a lane walks
 * the short rows at its junctions (a hub is slow, never wrong).  Checked on the device before anything is written, one flag word read
 * by the host, S2K_ERR_INVALID_ARG otherwise: row_off[0] == 0, non-decreasing, row_off[2 n_unitigs] == n_edges, every id below
 * 2 n_unitigs, uni_off strictly ascending (every unitig holds a member).  Twin symmetry is trusted (s2k_graph_unitigs checks it).
 * n_unitigs >= 2^31 is refused; n_unitigs == 0 needs n_edges == 0 and reads nothing.  d_dst may be NULL when n_edges == 0.  The
 * three totals are integer sums: the outputs are a function of the input, bit-identical from call to call.  Workspace: 32 B of the
 * context's grow-only count workspace.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_graph_simplify_mask(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                   const uint64_t *d_uni_off, const uint64_t *d_uni_count, uint32_t max_tip, uint32_t max_bubble,
                                   uint8_t *d_remove, uint64_t *n_tips, uint64_t *n_bubbles, uint64_t *n_removed);
/* The subgraph induced by the kept nodes of a graph (d_keys / d_counts: its node table, strictly ascending; d_edge_keys /
 * d_edge_counts: its edges, u << 32 | v strictly ascending, as s2k_graph_adjacency takes them).  Which nodes are kept comes from one
 * of two sources: d_node_keep (one byte per node, non-zero = kept), or, when d_node_keep is NULL, the unitig mask gathered inside
 * the call, keep[i] = !d_remove[d_node_unitig[i]] (d_node_unitig of s2k_graph_unitigs, d_remove of s2k_graph_simplify_mask over
 * n_unitigs unitigs; an entry >= n_unitigs is S2K_ERR_INVALID_ARG).
 * d_new_id[i] (n_nodes entries) = the kept nodes before i (ids in ascending old order), 0xFFFFFFFF for a removed node.  The new node
 * table is the kept (key, count) pairs: still strictly ascending, so s2k_table_create accepts it.  An edge is kept iff both its ends
 * are; its key becomes (2 new_id[u >> 1] + (u & 1)) << 32 | (2 new_id[v >> 1] + (v & 1)), its count goes with it.  The map is
 * monotone: the kept keys stay strictly ascending without a sort, and the subgraph of a twin-symmetric graph is twin-symmetric.
 * *n_nodes_out and *n_edges_out are always set.  Every output array may be NULL (all NULL: the sizes only); d_counts / d_edge_counts
 * may be NULL when their outputs are.  The arrays are written only when *n_nodes_out <= node_capacity (asked of d_keys_out /
 * d_counts_out) and *n_edges_out <= edge_capacity (of d_edge_keys_out / d_edge_counts_out), otherwise S2K_ERR_CAPACITY and nothing is
 * written.  An edge that names a node >= n_nodes is S2K_ERR_INVALID_ARG, found on the device before anything is written; the order
 * of keys is trusted.  Outputs must not overlap inputs.  n_nodes >= 2^31 is refused.  Workspace (the context's grow-only count
 * workspace): 0.2 B per node and per edge (a kept bit, and 4 B per 64 items and per tile of 2048 items), and 4 B per node when
 * d_new_id is NULL and edge outputs are asked for.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_graph_induced(s2k_ctx *ctx, const uint64_t *d_keys, const uint32_t *d_counts, uint64_t n_nodes, const uint64_t *d_edge_keys,
                             const uint32_t *d_edge_counts, uint64_t n_edges, const uint8_t *d_node_keep, const uint32_t *d_node_unitig,
                             const uint8_t *d_remove, uint64_t n_unitigs, uint32_t *d_new_id, uint64_t *d_keys_out, uint32_t *d_counts_out,
                             uint64_t node_capacity, uint64_t *d_edge_keys_out, uint32_t *d_edge_counts_out, uint64_t edge_capacity,
                             uint64_t *n_nodes_out, uint64_t *n_edges_out);
/* ---- bubbles that are not simple: bounded superbubbles popped on the unitig graph ---------------------------------
 * Input and notation: the compacted graph of s2k_graph_simplify_mask above (the CSR over the 2 T oriented unitigs, len[t], cnt[t],
 * succ, pred, in, out).
 * Source: an oriented unitig S with out(S) >= 2.
 * Traversal from S, a bounded Kahn walk (the shape of miniasm's asg_bub_pop1).  A list of discovered oriented unitigs is kept in
 * slots, in order of first discovery; S is in slot 0.  An entry W holds r, the in-edges of W not yet seen (it starts at in(W); S
 * starts at 0 whatever in(S) is); best, the largest sum of cnt over the interior unitigs of a path from S that reaches W, W itself not
 * included (sums are taken modulo 2^64); and bp, the predecessor that gave best, on equal sums the smaller oriented id.  An entry is
 * ready when r == 0 and it has not been expanded.  Repeat: expand the ready entry in the lowest slot, V: walk succ(V) in row order
 * with sum = best[V] + cnt[V] (best[S] + 0 for V == S), and for each W: a new W takes the next slot with r = in(W) - 1, best = sum,
 * bp = V; a W already in the list gets r -= 1 and, when sum > best[W] or (sum == best[W] and V < bp[W]), best = sum and bp = V.
 * Failure -- S has no bubble -- when: the expanded entry has out == 0 (a dead end inside); W >> 1 == S >> 1 (a cycle, or a hairpin
 * back); W ^ 1 is in the list (an inversion); W is new and the list already holds max_nodes + 2 entries; no entry is ready (some
 * entry still has r > 0: an in-edge from outside the list, or a cycle inside); an edge arrives at an entry whose r is already 0
 * (in(W) == 0 for a new W included: only a graph that is not twin-symmetric has such an edge).
 * Success: the first time that, after an expansion, exactly one entry is ready and every other entry is expanded; that entry is
 * the sink T, and it is not expanded.  The interior is the list without S and T.  The bubble exists iff the interior is not empty
 * (then 1 <= |interior| <= max_nodes by the bound on the list) and the sum of len over the interior is <= max_bubble (members, like
 * max_tip).  The kept path is T, bp[T], bp[bp[T]], ... back to S; the removable set is the interior unitigs not on it.  A bubble
 * whose removable set is empty (a direct edge S -> T beside one detour, say) does nothing and claims nothing.
 * Claims: two bubbles may share interior unitigs (a bubble and its twin seen from T ^ 1, a bubble inside another, bubbles that
 * overlap).  Every bubble with a non-empty removable set claims each of its interior unitigs t (the unitig, not the oriented
 * unitig): owner[t] = min(owner[t], S), S the oriented id of its source.  A bubble is applied iff owner[t] == S for its whole
 * interior; the others wait for a later round.  The smallest claiming source owns everything it claimed, so a round that finds a
 * bubble applies one and removes a unitig; a minimum does not depend on the order of the claims, so the outputs are a function of the
 * input.
 * Removal: unitig t is removed iff it is in the removable set of an applied bubble.
 * Invariants: a kept oriented unitig with out >= 1 keeps a successor (no new dead end); the kept graph is twin-symmetric (removal
 * is by unitig); the interior of an applied bubble has no edge to or from anything outside the bubble (an in-edge from outside keeps
 * its target from becoming ready, an out-edge puts its target into the list).
 *
 * s2k_graph_bubble_mask: d_remove[t] (one byte per unitig, 0 / 1; NULL: the totals only), *n_sources = the oriented unitigs with
 * out >= 2, *n_found = the sources whose bubble has a non-empty removable set, *n_applied = those of them that were applied,
 * *n_removed = the bytes set.  max_nodes from 1 to S2K_BUBBLE_MAX_NODES (0 or a larger value: S2K_ERR_INVALID_ARG, decided on the host);
 * max_bubble == 0 finds nothing.  One wave per source, a lane per list slot, at most S2K_BUBBLE_WAVES waves in a bounded grid; a row
 * is walked entry by entry (a hub is slow, never wrong: it fails once the list is full).  The traversal runs twice, for the claims
 * and again to apply.  Checked on the device before anything is written, as for s2k_graph_simplify_mask and with the same refusals
 * (n_unitigs >= 2^31; n_unitigs == 0 needs n_edges == 0 and reads nothing; d_dst may be NULL when n_edges == 0); twin symmetry is
 * trusted, and a graph without it gets an answer by the rules above, not a fault.  The totals are integer sums: bit-identical from
 * call to call.  Workspace (the context's grow-only count workspace): 14.4 B per unitig (the sources, their found bytes, owner, the
 * compaction's masks).  Runs on the context's stream; returns when the outputs are written. */
#define S2K_BUBBLE_MAX_NODES 62u
#define S2K_BUBBLE_WAVES 8192u
s2k_status s2k_graph_bubble_mask(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                 const uint64_t *d_uni_off, const uint64_t *d_uni_count, uint32_t max_nodes, uint32_t max_bubble,
                                 uint8_t *d_remove, uint64_t *n_sources, uint64_t *n_found, uint64_t *n_applied, uint64_t *n_removed);
/* ---- base-space sequences of the nodes and unitigs -----------------------------------------------------------
 * What rust-mdbg keeps per solid k-min-mer: the bases of one occurrence and two shifts; a unitig's sequence is each member's first
 * `shift` bases, then the whole last member.  Inputs per batch: what s2k_extract_device wrote WITH S2K_FLAG_WANT_MINIMIZERS (km_off,
 * hash, rev, mn_off, mn_j, mn_jend), the batch's d_bases / d_read_off, the order k, and the table whose keys are the nodes.
 * Item j of read r is made of the read's minimizers j .. j + k - 1, the triples mn_off[r] + j .. mn_off[r] + j + k - 1: a read with
 * n > 0 items has exactly n + k - 1 triples (src/lib.rs:231-258).
 * Ordinal of item x of a batch: ordinal_base + x, ordinal_base = the items of all earlier batches (the global item order).
 * Representative of node i: the occurrence (an item whose hash is key i, whatever its count) with the smallest ordinal.
 * Node record, all from the representative (r, j): B = the read's bytes mn_j[j] ..= mn_jend[j + k - 1] as they are in d_bases
 * (original space also in the Hpc modes), seq_len = |B|, rev = the item's rev, shift_fwd = mn_j[j + 1] - mn_j[j], shift_rev =
 * mn_jend[j + k - 1] - mn_jend[j + k - 2].
 * Oriented node u = 2 i + o: seq(u) = B and shift(u) = shift_fwd when o == rev, otherwise seq(u) = revcomp(B) and shift(u) =
 * shift_rev; revcomp reverses and maps ACGTacgt -> TGCAtgca, every other byte stays what it is.  shift(u) <= seq_len always.
 * Sequence of unitig t with kept-strand members m_0 .. m_(n-1): seq(m_0)[:shift(m_0)] + .. + seq(m_(n-2))[:shift(m_(n-2))] +
 * seq(m_(n-1)); the last member of a circular unitig too gives only its first shift bytes.  The twin strand is the reverse
 * complement by definition and is not stored.  Overlap of an edge that leaves the oriented node u (or the oriented unitig whose last
 * member, in its orientation, is u): seq_len(u) - shift(u), "<n>M" in GFA.
 * With reads that hold sequencing errors the occurrences of a node differ, so a stitched sequence is one consistent choice (the
 * earliest occurrence of every node), not a consensus -- as in rust-mdbg.  The same holds, also for error-free reads, where two
 * different k-min-mers share a 64-bit hash: they are one node, which takes the bytes of whichever occurs first.  Everything here is a
 * function of the input alone (its order included): bit-identical from call to call.
 *
 * s2k_table_representatives: d_rep[i] = min(d_rep[i], ordinal_base + x) over the items x of the batch whose hash is key i.  d_rep
 * (one uint64_t per key) is the caller's: filled with 0xFF bytes before the first batch, carried from batch to batch.  km_off and
 * hash of `in` required, km_off[0] == 0. */
s2k_status s2k_table_representatives(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint64_t ordinal_base, uint64_t *d_rep);
typedef struct s2k_node_seqs { /* device pointers; the five record arrays hold one entry per key of the table */
    uint64_t *seq_off;         /* where B starts in pool */
    uint32_t *seq_len;         /* 0: no record (the caller zero-initialises seq_len; a key whose d_rep is still all ones keeps 0) */
    uint32_t *shift_fwd;
    uint32_t *shift_rev;
    uint8_t *rev;
    uint8_t *pool;
    uint64_t pool_capacity;    /* bytes */
} s2k_node_seqs;
/* For every item of the batch that IS its node's representative (d_rep[node] == ordinal_base + x, d_rep complete: every batch has
 * been through s2k_table_representatives) the node's record is written and B copied to pool + pool_used + (the summed lengths of the
 * representatives before it in this batch, in item order): after the last batch the pool is ordered by representative ordinal.
 * *n_bytes = the bytes this batch adds, always set; the caller adds it to pool_used for the next batch.  Every key that occurs in
 * some batch has a record then.  nodes == NULL or nodes->pool == NULL asks for *n_bytes only; otherwise all five record arrays are
 * required, and pool_used + *n_bytes > pool_capacity is S2K_ERR_CAPACITY with nothing written.  Checked on the device before
 * anything is written, S2K_ERR_INVALID_ARG otherwise: km_off[0] == mn_off[0] == 0, neither decreases, in->mn_capacity covers
 * mn_off[n_reads], every read with n > 0 items has n + k - 1 triples (it catches a wrong k, or the triples of another call), every
 * position a representative uses lies inside its read and in order.  k < 2 is refused (no second minimizer), as are missing
 * km_off / hash / rev / mn_off / mn_j / mn_jend.  d_read_off is trusted to be the table s2k_extract_device validated.  Uses the
 * context's grow-only count workspace: 16 B per item.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_table_node_sequences(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t k, const uint8_t *d_bases,
                                    const uint64_t *d_read_off, uint64_t ordinal_base, const uint64_t *d_rep, const s2k_node_seqs *nodes,
                                    uint64_t pool_used, uint64_t *n_bytes);
/* The stitch: d_out[d_out_off[t] .. d_out_off[t + 1]) = the sequence of unitig t, for the unitigs (d_uni_off, d_members, d_circular,
 * n_unitigs) that s2k_graph_unitigs wrote over n_nodes nodes, whose records are `nodes` (pool_capacity bounds every read of the
 * pool).  d_overlap (may be NULL; 2 * n_unitigs entries) = the overlap that leaves each oriented unitig.  *n_bases is always set;
 * d_out_off (n_unitigs + 1 entries, may be NULL) and d_overlap are written whenever the call succeeds; d_out == NULL asks for them
 * and the size only; *n_bases > capacity with d_out given is S2K_ERR_CAPACITY and nothing at all is written.  d_out must be 16-byte
 * aligned (stores are 16 bytes wide).  Checked on the device before anything is written (S2K_ERR_INVALID_ARG): uni_off starts at 0,
 * ends at n_nodes, every unitig holds a member; every member names a node below n_nodes whose record has rev <= 1, both shifts <=
 * seq_len and its bytes inside the pool.  A node without a record (seq_len 0) contributes nothing.  Workspace: 12 B per member. */
s2k_status s2k_unitig_sequences(s2k_ctx *ctx, const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular,
                                uint64_t n_unitigs, uint64_t n_nodes, const s2k_node_seqs *nodes, uint64_t *d_out_off, uint8_t *d_out,
                                uint32_t *d_overlap, uint64_t capacity, uint64_t *n_bases);
/* ---- read paths: the reads threaded through the unitig graph ------------------------------------------------------
 * Node place.  For node i of a unitig decomposition (what s2k_graph_unitigs wrote) let t = node_unitig[i], p = node_pos[i], len =
 * uni_off[t + 1] - uni_off[t] and o = members[uni_off[t] + p] & 1.  The forward oriented node 2 i lies on the oriented unitig U0 =
 * 2 t + o at position q0 = o ? len - 1 - p : p; node 2 i + 1 lies on U0 ^ 1 at len - 1 - q0.  The record of node i is
 * { unitig = U0, pos = q0, len, circular = circular[t] }, 16 bytes.
 * Item place.  Item j of a read (hash h, strand rev) is solid iff h is in the table with a count of at least max(min_count, 1), the
 * rule of s2k_table_filter and s2k_table_edges.  Its place, from the record of node index(h): U = U0 ^ rev, q = rev ? len - 1 - q0 :
 * q0.
 * Step.  Item j + 1 continues item j iff they are consecutive items of the same read, both are solid, U(j + 1) == U(j), and either
 * q(j + 1) == q(j) + 1, or the unitig is circular, q(j) == len - 1 and q(j + 1) == 0.  A step is a maximal run of items each of which
 * continues the one before it; a read's path is its steps in item order; a non-solid item belongs to no step.  (A loop on a unitig of
 * one member gives two steps: a unitig of length 1 is never circular.)
 * Step record, one entry per array: unitig = U; pos = q of the first item; count = the number of items; item = the first item's
 * index in its read before filtering (the convention of s2k_solid_out.offset); flags bit 0 S2K_STEP_LINKED = the step's first item
 * is consecutive with a solid item of the same read: the read crosses a graph adjacency into this step, not a gap; start = in->start
 * of the first item, end = in->end of the last.
 * Paths are in minimizer space: the base-level alignment of a read to a unitig's sequence (a CIGAR) is out of scope; the coordinate
 * lift of a path to bases is s2k_paths_walks, below.
 *
 * Threading through a simplified graph needs no node map: make a table over the simplified graph's node keys (s2k_graph_induced
 * writes them strictly ascending, so s2k_table_create accepts them), take its unitigs and their places, and thread against those --
 * an item whose node was removed is not in that table and breaks the path like any other non-solid item. */
typedef struct s2k_node_place {
    uint32_t unitig;   /* the oriented unitig of the oriented node 2 i */
    uint32_t pos;      /* its position there */
    uint32_t len;      /* members of the unitig */
    uint32_t circular; /* 0 / 1 */
} s2k_node_place;
/* d_place[i] (n_nodes records, 16-byte aligned) from the arrays s2k_graph_unitigs wrote over n_nodes nodes and n_unitigs unitigs.
 * Checked on the device before anything is written, one flag word read by the host, S2K_ERR_INVALID_ARG otherwise: node_unitig[i] <
 * n_unitigs, the unitig's members lie inside [0, n_nodes] and it holds one, node_pos[i] < len, members[uni_off[t] + p] >> 1 == i.
 * n_nodes >= 2^31 is refused; n_nodes == 0 reads and writes nothing.  Workspace: 4 B of the context's grow-only count workspace.  Runs
 * on the context's stream; returns when the records are written. */
s2k_status s2k_unitig_node_places(s2k_ctx *ctx, const uint64_t *d_uni_off, const uint32_t *d_members, const uint32_t *d_node_unitig,
                                  const uint32_t *d_node_pos, const uint8_t *d_circular, uint64_t n_nodes, uint64_t n_unitigs,
                                  s2k_node_place *d_place);
#define S2K_STEP_LINKED 1u
typedef struct s2k_thread_out { /* device pointers; capacity in steps */
    uint64_t capacity;
    uint64_t *path_off; /* n_reads + 1, required: the steps of read r are [path_off[r], path_off[r + 1]) */
    uint32_t *unitig;   /* every step array may be NULL */
    uint32_t *pos;
    uint32_t *count;
    uint32_t *item;
    uint32_t *flags;
    uint32_t *start;
    uint32_t *end;
} s2k_thread_out;
/* The paths of the reads of `in` (km_off, hash and rev required, km_off[0] == 0; start / end optional: out->start / out->end must be
 * NULL when theirs is) through the unitigs whose places are d_place[0..n_nodes); node i is key i of the table, so n_nodes must equal
 * the table's number of keys (S2K_ERR_INVALID_ARG otherwise; a table of 2^31 keys or more is refused).  *n_steps is always set and
 * out->path_off always written; the step arrays are written only when *n_steps <= out->capacity, otherwise S2K_ERR_CAPACITY and
 * nothing is written to them; all NULL asks for the sizes only.  d_uni_items (may be NULL; one uint64_t per unitig, n_unitigs of
 * them): d_uni_items[U >> 1] += count for every step, by every call that returns S2K_OK (a sizes-only call included) -- the items
 * each unitig carries; the caller zeroes it, and it accumulates over batches.  One integer atomic per step: sums do not depend on
 * their order, so every output is a function of the input, bit-identical from call to call.  Checked on the device before anything
 * is written (S2K_ERR_INVALID_ARG): every record a solid item uses names a unitig below n_unitigs and a position inside it.  d_place
 * is otherwise trusted to be what s2k_unitig_node_places wrote.  Uses the context's grow-only count workspace (shared with
 * s2k_count_device_ex): about 8.4 B per input item.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_table_thread(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t min_count, const s2k_node_place *d_place,
                            uint64_t n_nodes, const s2k_thread_out *out, uint64_t *d_uni_items, uint64_t n_unitigs, uint64_t *n_steps);
/* ---- junction spans: which reads cross a unitig, and which repeats they resolve ------------------------------------
 * Inputs: the path arrays s2k_table_thread wrote (path_off, unitig, pos, count, flags of an s2k_thread_out; n_reads, n_steps), the CSR
 * over the 2 T oriented unitigs (d_row_off, d_dst, n_edges: what s2k_graph_adjacency writes from the keys of s2k_graph_unitig_edges;
 * twin-symmetric, every row strictly ascending) and d_uni_off, len[t] = uni_off[t + 1] - uni_off[t].
 * Edge index: the index of an edge in d_dst.  find(A, B) = the index of B in the row of A, or none.  For e = (A -> B), tw(e) =
 * find(B ^ 1, A ^ 1): the same adjacency read on the other strand.
 * Step s follows edge e iff all of these hold: s > path_off[r] (it is not its read's first step); flags[s] & S2K_STEP_LINKED; pos[s]
 * == 0; pos[s - 1] + count[s - 1] == len[unitig[s - 1] >> 1]; e = find(unitig[s - 1], unitig[s]) exists.  A linked step that follows
 * no edge is off-graph (a jump inside a unitig, or paths threaded against another graph than this CSR): it is counted, never an
 * error.  A circular unitig has an empty row in a valid graph, so it never qualifies.
 * Edge support: d_edge_support[e] += 1 for every step that follows e, and d_edge_support[tw(e)] += 1 when tw(e) != e (a hairpin is
 * its own twin: counted once).  On the reads a graph was built from, with the same min_count and min_edge_count 1, it equals the
 * graph's edge counts entry for entry.
 * Span: step s spans its unitig V = unitig[s] iff it follows an edge a, step s + 1 is of the same read and follows an edge b, and
 * count[s] == len[V >> 1] (V was traversed whole).  The span gives the key a << 32 | b and then the key of its twin, tw(b) << 32 |
 * tw(a): the same read on the other strand.  A span is never its own twin (tw(a) leaves V ^ 1, b leaves V), so every span gives
 * exactly two keys.  Keys come in step order, bit-identical from call to call.  Counting them (s2k_count_device_ex sorted, or an
 * s2k_counter over batches) gives the span table, count(a, b) == count(tw b, tw a).
 *
 * s2k_paths_spans: *n_keys, *n_followed (steps that follow an edge) and *n_off_graph are always set.  d_span_keys NULL asks for the
 * sizes only; *n_keys > capacity is S2K_ERR_CAPACITY and nothing is written, to the keys or to d_edge_support.  d_edge_support (may be
 * NULL; n_edges uint64_t) is the caller's: zeroed before the first batch, it accumulates over the calls that return S2K_OK (a
 * sizes-only call included).  Checked on the device before anything is written, one flag word read by the host, S2K_ERR_INVALID_ARG
 * otherwise: path_off[0] == 0, non-decreasing, path_off[n_reads] == n_steps; every unitig[s] < 2 n_unitigs; the row_off rules of
 * s2k_graph_simplify_mask, every id below 2 n_unitigs; uni_off strictly ascending.  paths->path_off is required, and with n_steps > 0
 * paths->unitig, pos, count and flags.  n_unitigs >= 2^31 and n_edges >= 2^32 (a key holds two edge indices) are refused.  Twin
 * symmetry and the order inside a row are trusted.  Slots come from ballots and scans and the only atomics are integer sums: every
 * output is a function of the input.  Uses the context's grow-only count workspace: about 4.2 B per step.  Runs on the context's
 * stream; returns when the outputs are written. */
s2k_status s2k_paths_spans(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint64_t *d_row_off,
                           const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, uint64_t n_unitigs, uint64_t *d_span_keys,
                           uint64_t capacity, uint64_t *d_edge_support, uint64_t *n_keys, uint64_t *n_followed, uint64_t *n_off_graph);
/* Resolution, decided per oriented unitig V from a span table (d_span_keys strictly ascending, d_span_counts) and min_support (0 and
 * 1 both mean 1).  sup(a, b) = the count of the key a << 32 | b, or 0; a pair is supported iff sup >= min_support.  in(V) = out(V ^
 * 1); the in-edges of V are the twins of the edges that leave V ^ 1.  V is a candidate iff in(V) >= 2 and out(V) >= 2.  V is resolved
 * iff it is a candidate, in(V) == out(V), no predecessor or successor is of V's own unitig, and the supported pairs are a perfect
 * matching: every in-edge has exactly one supported out-edge and every out-edge exactly one supported in-edge.  Unitig t is resolved
 * iff both 2 t and 2 t + 1 are (with a twin-symmetric span table they agree).
 * d_resolved[t] (may be NULL): one byte per unitig, 0 / 1.  d_partner[e] (may be NULL; n_edges entries): the out-edge matched to e
 * when e enters a resolved oriented unitig, S2K_NO_PARTNER otherwise; partner[tw(partner[a])] == tw(a).  *n_candidates and
 * *n_resolved, counted in unitigs, are always set.  Checked on the device before anything is written (S2K_ERR_INVALID_ARG): the
 * row_off rules and ids as above; span keys strictly ascending, both halves < n_edges, the out half in the row of the unitig that
 * the in half enters.  n_unitigs >= 2^31 and n_edges >= 2^32 are refused.  One lane per oriented unitig; a hub is slow (quadratic in
 * its degree), never wrong.  Workspace: 32 B of the context's grow-only count workspace.  Runs on the context's stream; returns when
 * the outputs are written.  Duplicating a resolved unitig (the graph surgery) is s2k_graph_untangle, below. */
#define S2K_NO_PARTNER 0xFFFFFFFFu
s2k_status s2k_graph_resolve_mask(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                                  const uint64_t *d_span_keys, const uint32_t *d_span_counts, uint64_t n_spans, uint32_t min_support,
                                  uint8_t *d_resolved, uint32_t *d_partner, uint64_t *n_candidates, uint64_t *n_resolved);
/* ---- untangling: resolved unitigs duplicated, the contigs expanded to node members -------------------------------------
 * Input: the CSR over the 2 T oriented unitigs (d_row_off, d_dst, n_edges) with d_resolved[T] and d_partner[n_edges] as
 * s2k_graph_resolve_mask wrote them for that CSR; tw(e) as above.
 * Copies: deg(t) = out(2 t) for a resolved t (it equals in(2 t)); ncopies(t) = deg(t) if t is resolved, otherwise 1; copy_off[t] = the
 * copies of all unitigs below t (T + 1 entries); T' = copy_off[T]; origin[c] = t for copy_off[t] <= c < copy_off[t + 1]; oriented copy
 * C = 2 c + s.
 * Which copy an edge uses.  For a resolved t let base = row_off[2 t + 1].  Copy j is the copy whose reverse strand leaves over edge
 * base + j, the j-th entry of the row of 2 t + 1: its forward strand is entered by a_j = tw(base + j) and leaves over partner[a_j],
 * its reverse strand is entered by tw(partner[a_j]).  An edge e = (A -> B) picks copy index jA of its source unitig, 0 when A >> 1 is
 * not resolved; A odd: jA = e - base(A >> 1); A even: jA = partner[tw(e)] - base(A >> 1) (from partner[tw(partner[a])] == tw(a)).  It
 * picks copy index jB of its destination unitig, 0 when B >> 1 is not resolved; B even: jB = tw(e) - base(B >> 1); B odd: jB =
 * partner[e] - base(B >> 1).  Every old edge becomes exactly one new edge: A' = 2 (copy_off[A >> 1] + jA) + (A & 1), B' likewise,
 * key A' << 32 | B'.  The new graph has n_edges edges over T' copies and is twin-symmetric; each strand of a copy of a resolved unitig
 * has in = out = 1, so the compaction (s2k_graph_unitigs over the T' copies) joins it to what it was matched with.
 * Copy count (written only when d_uni_count, d_edge_counts and d_copy_count are all given): an unresolved unitig keeps cnt[t]; copy j
 * of a resolved t gets floor(cnt[t] * w_j / S), w_j = edge_counts[a_j], S = the sum of the w_i -- exact, no floating point: (cnt / S)
 * * w_j + ((cnt % S) * w_j) / S with a 128-bit product; S == 0 gives 0.  The copies' counts add up to at most deg - 1 less than cnt[t].
 *
 * s2k_graph_untangle: d_copy_off (T + 1), d_origin (T'), d_copy_count (T'), d_keys (n_edges, strictly ascending:
 * s2k_graph_adjacency(d_keys, n_edges, T') takes them as they are) and d_src_edge (n_edges; the old edge key j came from: the caller
 * gathers edge counts with it); each may be NULL.  *n_copies = T' and *n_duplicated (the resolved unitigs) are always set.  The arrays
 * are written only when *n_copies <= capacity, otherwise S2K_ERR_CAPACITY and nothing is written; all NULL asks for the sizes only.
 * One lane per unitig and a scan give copy_off, one lane per new oriented copy and a scan the new row offsets, one lane per new
 * oriented copy writes its row: a copy strand of a resolved unitig its one edge, an unresolved A its old row with every destination
 * mapped.  The map is monotone between unitigs but not inside a row (edges of A to both 2 t and 2 t + 1 of a resolved t can swap), so
 * a row's keys are placed by repeated selection (quadratic in a hub's degree: slow, never wrong).  No sort, no atomic on an output:
 * every output is a function of the input, bit-identical from call to call.  A graph with nothing resolved gives the identity:
 * origin[c] = c, the keys equal to the input's.
 * Checked on the device before anything is written, one flag word read by the host, S2K_ERR_INVALID_ARG otherwise: the row_off rules
 * of s2k_graph_simplify_mask, every id below 2 n_unitigs; d_resolved bytes 0 or 1; a resolved t has out(2 t) == out(2 t + 1) >= 2;
 * each in-edge of 2 t and of 2 t + 1 has its partner in the row of the strand it enters; no two in-edges share a partner;
 * partner[tw(partner[a])] == tw(a).  Twin symmetry elsewhere and the order inside a row are trusted.  n_unitigs >= 2^31, n_edges >=
 * 2^32 and T' >= 2^31 are refused; n_unitigs == 0 needs n_edges == 0 and reads nothing.  d_dst and d_partner may be NULL when n_edges
 * == 0.  Outputs must not overlap inputs.  Workspace (the context's grow-only count workspace), sized by T' <= T + n_edges / 2: 40 B
 * per unitig and 14 B per edge.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_graph_untangle(s2k_ctx *ctx, const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, uint64_t n_unitigs,
                              const uint8_t *d_resolved, const uint32_t *d_partner, const uint64_t *d_uni_count, const uint32_t *d_edge_counts,
                              uint64_t *d_copy_off, uint32_t *d_origin, uint64_t *d_copy_count, uint64_t *d_keys, uint64_t *d_src_edge,
                              uint64_t capacity, uint64_t *n_copies, uint64_t *n_duplicated);
/* The contigs of the untangled graph as node members.  Input: the outer decomposition (d_outer_off, d_outer_members,
 * d_outer_circular: the uni_off / members / circular that s2k_graph_unitigs wrote with the n_copies copies as its nodes, n_contigs
 * unitigs), d_origin of s2k_graph_untangle, and the inner decomposition (d_uni_off, d_members, d_circular of the n_unitigs unitigs
 * over n_nodes nodes).
 * Every output member slot m is a node instance.  An outer member C = 2 c + s contributes the members of unitig origin[c]: in order
 * for s == 0, reversed and each ^ 1 for s == 1; so instance ids run in path order.  d_node_origin[m] = the old node id;
 * d_members_out[m] = 2 m + (the old oriented node's orientation bit); d_node_unitig[m] = its contig; d_node_pos[m] = its position in
 * the contig; d_uni_off_out has n_contigs + 1 entries, the last one M, the total of instances; d_circular_out[t] = outer circular, or
 * the contig is a single copy whose origin is circular.  The result is a valid input of s2k_unitig_sequences, s2k_unitig_node_places
 * and the GFA writers with n_nodes = M, the node records gathered through d_node_origin.
 * *n_members = M is always set; every output may be NULL (all NULL: the size only); the arrays are written only when M <= capacity,
 * otherwise S2K_ERR_CAPACITY and nothing is written.  Checked on the device before anything is written (S2K_ERR_INVALID_ARG): both
 * uni_off arrays ascend strictly from 0 to n_copies / n_nodes; every outer member is below 2 n_copies; every origin it names is
 * below n_unitigs.  n_copies, n_nodes or M >= 2^31 are refused; n_copies == 0 reads nothing.  Piece lengths by one lane per outer
 * member, a scan, then an output-ordered write: consecutive lanes take consecutive slots.  Workspace: 16 B per copy.  Runs on the
 * context's stream; returns when the outputs are written. */
s2k_status s2k_unitig_expand(s2k_ctx *ctx, const uint64_t *d_outer_off, const uint32_t *d_outer_members, const uint8_t *d_outer_circular,
                             uint64_t n_contigs, uint64_t n_copies, const uint32_t *d_origin, const uint64_t *d_uni_off, const uint32_t *d_members,
                             const uint8_t *d_circular, uint64_t n_unitigs, uint64_t n_nodes, uint64_t *d_uni_off_out, uint32_t *d_members_out,
                             uint32_t *d_node_unitig, uint32_t *d_node_pos, uint8_t *d_circular_out, uint32_t *d_node_origin, uint64_t capacity,
                             uint64_t *n_members);
/* ---- read walks with base coordinates: the coordinate lift of the minimizer-space paths -------------------------------
 * Member offsets.  For the unitigs (d_uni_off, d_members, d_circular) over nodes with records `nodes`, member_off[x] (one uint64_t per
 * member slot x, n_nodes of them) is where the piece of slot x starts in the concatenated output of s2k_unitig_sequences; out_off[t] is
 * as that call writes it, L[t] = out_off[t + 1] - out_off[t]; for slot p of unitig t with oriented node m, o_p = member_off[uni_off[t] +
 * p] - out_off[t] and e_p = o_p + seq_len(m >> 1).
 * Base interval [lo, hi) of position q of the oriented unitig U = 2 t + s, len = the members of t, on the strand of U:
 *   s == 0: p = q, lo = o_p, hi = min(e_p, L[t]) (representatives of erroneous reads need not be consistent: the min keeps hi inside);
 *   s == 1: p = len - 1 - q, lo = L[t] - min(e_p, L[t]), hi = L[t] - o_p (the twin strand is the reverse complement by definition).
 * On a circular unitig no min is applied, so hi may pass L[t]: the last members reach round into the first.  There, on s == 1, L[t] -
 * e_p would be negative where e_p > L[t]; lo and hi are both raised by w = the multiple of L[t] that brings lo into [0, L[t]) (w = e_p
 * when L[t] == 0), w = 0 elsewhere.
 * Walk.  A walk is a maximal run of consecutive steps of one read in which every step after the first follows an edge, "follows an
 * edge" exactly as for s2k_paths_spans above, against the CSR over the oriented unitigs.  A step that is not linked, is linked but
 * off-graph, or is its read's first step starts a walk; every step belongs to exactly one walk; a read's walks are in step order.
 * Walk record, one entry per array: first_step, n_steps; items = the sum of count over its steps; qstart = start of the first step;
 * qend = end of the last step + 1 -- in->end is the index of the last base an item covers (inclusive, s2k_kminmer.end), the record is
 * half-open; adv(U) = L[U >> 1] - min(overlap[U], L[U >> 1]) with overlap the d_overlap of s2k_unitig_sequences; path_len = the sum
 * of adv(U) over all steps but the last + L of the last; path_start = lo of (U, pos) of the first step; path_end = the same sum of
 * adv + hi of (U, pos + count - 1) of the last step; flags bit 0 S2K_WALK_CIRCULAR = the walk lies on a circular unitig.  Such a walk
 * is one step (a circular unitig has no edges) and may go round more than once: with last = pos + count - 1, path_end = w(pos) + (last /
 * len) * L + the unraised hi of (U, last % len), i.e. path_start + the stitched length of its items; it may exceed path_len = L.
 * Elsewhere path_start <= path_end <= path_len.  The stitched path of a walk is the unitig sequences on the walk's strands, each after
 * the first without the overlap[U] bases of the one before it; on error-free reads read[qstart, qend) equals its bases [path_start,
 * path_end).  This is exact arithmetic on records, not an alignment: there is no CIGAR (s2k_walks_targets and s2k_align_pairs, below,
 * align a walk to its path). */
s2k_status s2k_unitig_member_offsets(s2k_ctx *ctx, const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular,
                                     uint64_t n_unitigs, uint64_t n_nodes, const s2k_node_seqs *nodes, uint64_t *d_member_off,
                                     uint64_t *d_out_off, uint32_t *d_overlap, uint64_t *n_bases);
/* The passes of s2k_unitig_sequences up to its copy kernel: d_member_off (n_nodes entries), d_out_off (n_unitigs + 1) and d_overlap (2
 * n_unitigs) as defined above, each may be NULL; *n_bases is always set; nodes->pool is not read.  The same inputs are checked in the
 * same way (S2K_ERR_INVALID_ARG, nothing written).  Workspace: 12 B per member. */
#define S2K_WALK_CIRCULAR 1u
#define S2K_NO_EDGE 0xFFFFFFFFu
typedef struct s2k_walk_out { /* device pointers, each may be NULL; capacity in walks */
    uint64_t capacity;
    uint64_t *walk_off;   /* n_reads + 1: the walks of read r are [walk_off[r], walk_off[r + 1]) */
    uint64_t *first_step;
    uint32_t *n_steps;
    uint64_t *items;
    uint32_t *qstart;
    uint32_t *qend;
    uint64_t *path_len;
    uint64_t *path_start;
    uint64_t *path_end;
    uint32_t *flags;
    uint32_t *edge;       /* n_steps entries, one per STEP: the index of the edge the step follows, S2K_NO_EDGE when none */
} s2k_walk_out;
/* The walks of the paths s2k_table_thread wrote (path_off, unitig, pos, count, flags; start / end when out->qstart / out->qend are
 * wanted) over the CSR of the oriented unitigs, lifted with d_member_off, d_out_off, d_overlap (s2k_unitig_member_offsets), d_seq_len
 * (the seq_len of the node records) and d_members.  d_circular is needed beside the arrays of the issue's draft: a step on a circular
 * unitig may pass its last member.  *n_walks, *n_followed and *n_off_graph (as s2k_paths_spans) are always set.  out NULL, or none of
 * the record arrays given, asks for the sizes; walk_off and edge are written whenever the call returns S2K_OK; *n_walks >
 * out->capacity with a record array given is S2K_ERR_CAPACITY and nothing at all is written.  Checked on the device before anything is
 * written, one flag word read by the host, S2K_ERR_INVALID_ARG otherwise: the rules of s2k_paths_spans; every step has count >= 1,
 * pos < len and, unless its unitig is circular, pos + count <= len; uni_off ascends strictly from 0 to n_nodes; every member < 2
 * n_nodes; out_off does not decrease; every member_off lies inside [out_off[t], out_off[t + 1]] of its unitig; L[t] < 2^32 (advances
 * are scanned as 32-bit inputs; a path's 64-bit sums are never narrowed).  n_unitigs >= 2^31, n_edges >= 2^32 and n_nodes >= 2^31 are
 * refused.  d_seq_len and the contents of d_overlap are trusted.  qend wraps for an end of 2^32 - 1, which no read of s2k_extract has.
 * Heads and tails of walks come from ballots and scans, sums from prefix differences; there is no atomic on an output: every output
 * is a function of the input, bit-identical from call to call.  Uses the context's grow-only count workspace: about 24.4 B per step.
 * Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_paths_walks(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint64_t *d_row_off,
                           const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular, uint64_t n_unitigs,
                           const uint64_t *d_member_off, const uint64_t *d_out_off, const uint32_t *d_overlap, const uint32_t *d_seq_len,
                           const uint32_t *d_members, uint64_t n_nodes, const s2k_walk_out *out, uint64_t *n_walks, uint64_t *n_followed,
                           uint64_t *n_off_graph);
/* ---- bridged read paths: error gaps closed along the graph ---------------------------------------------------------
 * Inputs: the path arrays s2k_table_thread wrote (path_off, unitig, pos, count, item and flags are required with n_steps > 0; start and
 * end are optional, and out->start / out->end must be NULL when theirs is), the CSR over the oriented unitigs (d_row_off, d_dst,
 * n_edges), d_uni_off, d_circular, n_unitigs, and the limits max_gap and max_slip, in items.  find(A, B) as for s2k_paths_spans.
 * Join.  For step s that is not its read's first step let a = unitig[s - 1], b = unitig[s], endp = pos[s - 1] + count[s - 1], la = the
 * members of a's unitig, gi = item[s] - (item[s - 1] + count[s - 1]): the read's items between the two steps.  join[s] is decided in
 * this order: it is 0 if either unitig is circular; if a == b and pos[s] >= endp the kind is 1 (the same unitig) and gp = pos[s] -
 * endp; otherwise, if find(a, b) exists, the kind is 2 (across one edge) and gp = (la - endp) + pos[s]; otherwise it is 0.  The kind
 * stands iff gi <= max_gap, gp <= max_gap and |gi - gp| <= max_slip; otherwise join[s] = 0.  A read's first step has join 0.  A step
 * that already follows an edge is kind 2 with gi = gp = 0 and comes out unchanged; a == b going backwards is kind 2 only over a loop
 * edge.
 * Output steps.  A run is a maximal sequence of steps s_a .. s_b of one read with join == 1 on all but the first; every run gives one
 * output step, in step order: unitig = unitig[s_a]; pos = 0 if join[s_a] == 2, else pos[s_a]; count = endpos - pos, where endpos = the
 * members of the unitig if step s_b + 1 is of the same read and join[s_b + 1] == 2, else pos[s_b] + count[s_b]; item = item[s_a]; flags
 * = flags[s_a] | (join[s_a] == 2 ? S2K_STEP_LINKED : 0); start = start[s_a]; end = end[s_b]; matched = the sum of the run's input
 * counts.  So in bridged paths count is "positions covered", the gaps included, and matched is "k-min-mers really found" (matched ==
 * count on paths nothing was bridged in); item + count may pass the next step's item by up to max_slip per join.  Downstream the
 * bridged paths are paths like any other: s2k_paths_spans and s2k_paths_walks take them as they are, and a walk's `items` over them
 * counts positions, not found k-min-mers.
 * Not done: a wholly missing unitig between two steps (two edges) is not bridged; a gap is judged in items only, with no base-space
 * plausibility check (start / end are carried, not compared); steps on circular unitigs are never joined.
 *
 * s2k_paths_bridge: *n_out_steps, *n_merged (joins of kind 1) and *n_bridged (joins of kind 2 with gi + gp > 0) are always set.
 * out->path_off (required, n_reads + 1) and d_join (may be NULL; one byte per input step) are written whenever the call returns
 * S2K_OK.  The step arrays of `out` (each may be NULL) and d_matched (may be NULL; one uint32_t per output step) are written only when
 * *n_out_steps <= out->capacity; otherwise S2K_ERR_CAPACITY and nothing at all is written; all of them NULL asks for the sizes only.
 * Outputs must not overlap inputs.  Checked on the device before anything is written, one flag word read by the host,
 * S2K_ERR_INVALID_ARG otherwise: the path and CSR rules of s2k_paths_walks (path_off from 0 to n_steps without decreasing; every unitig
 * < 2 n_unitigs; count >= 1, pos < len and, unless the unitig is circular, pos + count <= len; the row_off rules, every id below 2
 * n_unitigs; uni_off strictly ascending), no unitig of 2^32 members or more, and item[s] >= item[s - 1] + count[s - 1] inside a read,
 * so that gi cannot wrap.  n_unitigs >= 2^31 and n_edges >= 2^32 are refused.  Twin symmetry and the order inside a row are trusted.
 * Heads and tails of runs come from ballots and scans, matched from a prefix difference; there is no atomic on an output: every
 * output is a function of the input, bit-identical from call to call.  Uses the context's grow-only count workspace: about 9.4 B per
 * step.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_paths_bridge(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint64_t *d_row_off,
                            const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular, uint64_t n_unitigs,
                            uint32_t max_gap, uint32_t max_slip, const s2k_thread_out *out, uint32_t *d_matched, uint8_t *d_join,
                            uint64_t *n_out_steps, uint64_t *n_merged, uint64_t *n_bridged);
/* ---- read paths lifted onto the untangled contigs -----------------------------------------------------------------------
 * Where every copy lies.  Input: the outer decomposition that s2k_graph_unitigs wrote over the n_copies copies of s2k_graph_untangle
 * (d_outer_off, d_outer_members, d_outer_circular, n_contigs), d_origin of s2k_graph_untangle, and d_uni_off, d_circular of the n_unitigs
 * unitigs the copies were made of.  Let the outer member at slot p of contig t be C = 2 c + s, f = the members of all pieces before slot
 * p in that contig, m = the members of unitig origin[c], Lc = the node instances of contig t as s2k_unitig_expand counts them.
 * d_copy_place[c] (n_copies records of s2k_node_place, 16-byte aligned) says where the forward oriented copy 2 c lies: unitig = 2 t + s,
 * the oriented contig; pos = s ? Lc - f - m : f; len = Lc; circular = what s2k_unitig_expand writes to circular_out[t].
 * Checked on the device before anything is written, one flag word read by the host, S2K_ERR_INVALID_ARG otherwise: the rules of
 * s2k_unitig_expand on the same arrays (the outer uni_off ascends strictly from 0 to n_copies, the inner one strictly from 0 -- its
 * end cannot be checked without n_nodes; every outer member is below 2 n_copies; every origin it names is below n_unitigs), every copy
 * is named by exactly one outer member (so every record has one writer), and no unitig or contig has 2^32 members or more.  n_copies
 * >= 2^31 is refused; n_copies == 0 reads and writes nothing.  One lane per outer member for the piece lengths, a scan, one lane per
 * outer member to write, its contig by a binary search of d_outer_off.  No atomic on an output.  Workspace: 16 B per copy of the
 * context's grow-only count workspace.  Runs on the context's stream; returns when the records are written. */
s2k_status s2k_unitig_copy_places(s2k_ctx *ctx, const uint64_t *d_outer_off, const uint32_t *d_outer_members, const uint8_t *d_outer_circular,
                                  uint64_t n_contigs, uint64_t n_copies, const uint32_t *d_origin, const uint64_t *d_uni_off, const uint8_t *d_circular,
                                  uint64_t n_unitigs, s2k_node_place *d_copy_place);
/* The lift.  Inputs: the path arrays of an s2k_thread_out on the OLD unitig graph (path_off, unitig, pos, count, item and flags are
 * required with n_steps > 0; start and end are optional, and out->start / out->end must be NULL when theirs is); d_matched_in (may be
 * NULL), the matched of bridged paths; the old CSR (d_row_off, d_dst, n_edges) with d_uni_off, d_circular, n_unitigs; d_resolved and
 * d_partner as s2k_graph_untangle took them and d_copy_off (n_unitigs + 1) as it wrote it; d_copy_place (n_copies records) from the
 * call above; n_contigs.  "Step s follows edge e" and tw(e) are exactly as for s2k_paths_spans; len[t], base(t) = row_off[2 t + 1] and
 * ncopies(t) = copy_off[t + 1] - copy_off[t] as for s2k_graph_untangle.
 * Copy of a step.  Step s lies on U = unitig[s], t = U >> 1.  If t is not resolved, j = 0.  Otherwise, if s follows an edge e (it enters
 * U): j = tw(e) - base(t) for U even, j = partner[e] - base(t) for U odd -- jB of s2k_graph_untangle.  Otherwise, if step s + 1 is of
 * the same read and follows an edge e' (it leaves U): j = e' - base(t) for U odd, j = partner[tw(e')] - base(t) for U even -- jA.
 * Otherwise the step is ambiguous: it lies on a duplicated unitig and the read shows neither the way in nor the way out; it is dropped
 * and counted in *n_dropped.  Where both edges exist and give different j the entering edge wins and the step is counted in
 * *n_conflicts: the read crossed the repeat by a pair the matching did not keep, and in the new graph its next step follows no edge.
 * A j outside [0, ncopies(t)) is possible only where the trusted symmetry does not hold; it becomes 0, so that every access stays
 * inside the arrays (the rule of s2k_graph_untangle).  c = copy_off[t] + j.
 * Mapped position.  With rec = copy_place[c], m = len[t], su = U & 1: V = rec.unitig ^ su; q' = su ? rec.len - rec.pos - m + pos[s] :
 * rec.pos + pos[s].
 * Join.  join[s] = 1 iff steps s - 1 and s are of one read, both are kept, s follows an edge, V(s) == V(s - 1) and q'(s) == q'(s - 1) +
 * count[s - 1] -- on a circular contig taken modulo rec.len, the wrap s2k_table_thread allows on a circular unitig; otherwise 0.  This
 * holds exactly when the new edge between the two copies was compacted into a contig: there is one old edge per pair (A, B) and every
 * old edge becomes exactly one new edge, between the copies this rule picks (jA, jB), so the step follows THAT new edge; the compaction
 * joins two copies only along an edge, in path order, so two copies lie side by side on one contig strand, the second beginning where
 * the first ends, iff the compaction went along that edge (a contig of one copy joined to itself end to end is circular, a cycle of
 * copies closes modulo its length).
 * Output steps.  One output step per maximal run s_a .. s_b of kept steps with join == 1 on all but the first, in step order: unitig =
 * V(s_a); pos = q'(s_a); count = the sum of the run's counts (modulo 2^32; a run on a contig that is not circular stays inside it); item
 * = item[s_a]; flags = flags[s_a]; start = start[s_a]; end = end[s_b]; matched = the sum of matched_in over the run, or of count when
 * d_matched_in is NULL.  A dropped step is in no run; by its definition the step after it follows no edge, so heads and tails pair one
 * to one.  The lifted paths are paths on the contig graph like any other: s2k_paths_spans, s2k_paths_walks and s2k_paths_bridge take
 * them as they are.  The item order is not checked (bridged paths may overlap by max_slip).
 *
 * s2k_paths_lift: *n_out_steps, *n_merged (joins), *n_dropped and *n_conflicts are always set.  out->path_off (required, n_reads + 1),
 * d_step_copy (may be NULL; one uint32_t per INPUT step: the copy c, S2K_NO_COPY when dropped) and d_join (may be NULL; one byte per
 * input step) are written, and d_contig_items (may be NULL; n_contigs uint64_t: [V >> 1] += count for every output step; the caller
 * zeroes it and it accumulates over batches, the rule of d_uni_items of s2k_table_thread, a sizes-only call included) gains, whenever
 * the call returns S2K_OK.  The step arrays of `out` (each may be NULL) and d_matched (may be NULL; one uint32_t per output step) are
 * written only when *n_out_steps <= out->capacity; otherwise S2K_ERR_CAPACITY and nothing at all is written; all of them NULL asks for
 * the sizes only.  Outputs must not overlap inputs.  Checked on the device before anything is written, one flag word read by the
 * host, S2K_ERR_INVALID_ARG otherwise: the path and CSR rules of s2k_paths_bridge but for the item order; d_resolved bytes 0 or 1;
 * copy_off from 0, copy_off[n_unitigs] == n_copies, copy_off[t + 1] - copy_off[t] == out(2 t) >= 1 for a resolved t and 1 otherwise;
 * every copy record has unitig < 2 n_contigs, pos + len[t] <= len and circular 0 or 1.  n_unitigs >= 2^31, n_copies >= 2^31 and
 * n_edges >= 2^32 are refused.  Twin symmetry, the order inside a row and the partner rules that s2k_graph_untangle checks are
 * trusted.  Kept steps, heads and tails of runs come from ballots and scans, the sums from prefix differences; the only atomic on an
 * output is the integer sum into d_contig_items (one per kept input step: the steps of a run lie on one contig): every output is a
 * function of the input, bit-identical from call to call.  Uses the context's grow-only count workspace: about 21.4 B per step (join
 * 1, copy 4, the prefixes of count and matched_in 8 each, two masks).  Runs on the context's stream; returns when the outputs are
 * written. */
#define S2K_NO_COPY 0xFFFFFFFFu
s2k_status s2k_paths_lift(s2k_ctx *ctx, uint64_t n_reads, const s2k_thread_out *paths, uint64_t n_steps, const uint32_t *d_matched_in,
                          const uint64_t *d_row_off, const uint32_t *d_dst, uint64_t n_edges, const uint64_t *d_uni_off, const uint8_t *d_circular,
                          uint64_t n_unitigs, const uint8_t *d_resolved, const uint32_t *d_partner, const uint64_t *d_copy_off,
                          const s2k_node_place *d_copy_place, uint64_t n_copies, uint64_t n_contigs, const s2k_thread_out *out, uint32_t *d_matched,
                          uint32_t *d_step_copy, uint8_t *d_join, uint64_t *d_contig_items, uint64_t *n_out_steps, uint64_t *n_merged,
                          uint64_t *n_dropped, uint64_t *n_conflicts);
/* ---- majority-vote representatives: every node takes its best-supported occurrence ---------------------------------
 * The sequence calls above take the bytes of a node's earliest occurrence.  These calls choose another ordinal for d_rep: the
 * occurrence that reads like most of the others.  No alignment, no new record format: s2k_table_node_sequences, the stitch and
 * everything after them take the voted d_rep as they take the earliest one.  Inputs per batch as for s2k_table_node_sequences.
 * Readings.  An occurrence x of node i (an item whose hash is key i, whatever its count) with bytes B, rev, shift_fwd and shift_rev
 * as defined above has three readings, each with a tag:
 *   whole:        B if rev == 0, else revcomp(B)                                             tag 4 i
 *   forward end:  B[:shift_fwd], what the stitch takes from the oriented node 2 i + rev      tag 4 i + 2 + rev
 *   reverse end:  revcomp(B[len - shift_rev:]), what it takes from 2 i + (1 - rev)           tag 4 i + 2 + (1 - rev)
 * Fingerprint of a byte string s of length n: F(s) = sum over j of (s_j + 1) * M^(n - 1 - j) mod 2^64, M = 0x9E3779B97F4A7C15 (the
 * Horner loop F = F * M + s_j + 1 from F = 0; the empty string has F = 0).  F(a || b) = F(a) * M^|b| + F(b).
 * Vote key of a reading s with tag g: mix64(F(s) ^ mix64(g)), mix64 the splitmix64 finaliser: z = (z ^ (z >> 30)) *
 * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; z ^ (z >> 31).  (Mixed so that a count's radix partition sees
 * uniform top bits even for a graph of a few hundred nodes.)
 * votes(key) = the number of occurrences, over all batches, that gave that key, those of nodes that are not solid included.  The
 * score of x is the pair (votes(whole), votes(forward end) + votes(reverse end)), compared lexicographically; the voted representative
 * of node i is its occurrence with the largest score, the smallest global ordinal among equals.  In the packed word below the first
 * number saturates at 2047 and the second at 4095.  A fingerprint collision only adds a vote to another reading.  With error-free
 * reads all occurrences of a node read the same unless two k-min-mers share its hash, so the voted representative is the earliest.
 * Protocol: s2k_table_vote_keys per batch into a counter (s2k_counter_add); s2k_counter_finish with min_count 1 and s2k_table_create
 * give the vote table; s2k_table_vote_representatives per batch with the same ordinal_base rule as s2k_table_representatives;
 * s2k_vote_ordinals once.
 *
 * s2k_table_vote_keys: d_keys = the three vote keys (whole, forward end, reverse end) of every item of the batch whose hash is in the
 * table, in item order.  *n_keys is always set; d_keys NULL asks for the size only (d_bases may then be NULL); *n_keys > capacity is
 * S2K_ERR_CAPACITY and nothing is written.  Checked on the device before anything is written, S2K_ERR_INVALID_ARG otherwise: what
 * s2k_table_node_sequences checks, but for every item of the table, not only the representatives: km_off[0] == mn_off[0] == 0,
 * km_off / mn_off / read_off do not decrease, mn_capacity covers mn_off[n_reads], every read with n > 0 items has n + k - 1 triples,
 * every position an item uses lies inside its read and in order.  k < 2 is refused.  Every base of the batch is read twice (once
 * per pass of the two-pass fingerprint scan, both orientations from the same registers) whatever k is, and an item reads at most 15
 * more bytes at each of its five positions; no lane walks a node's bytes.  Workspace (the context's grow-only count workspace): 4.2 B
 * per item and 1 B per base.  Keys come from ballots and scans: bit-identical from call to call.  Runs on the context's stream;
 * returns when the outputs are written. */
s2k_status s2k_table_vote_keys(s2k_table *t, uint64_t n_reads, const s2k_device_out *in, uint32_t k, const uint8_t *d_bases,
                               const uint64_t *d_read_off, uint64_t *d_keys, uint64_t capacity, uint64_t *n_keys);
/* d_best[i] = max(d_best[i], w << 52 | e << 40 | (2^40 - 1 - (ordinal_base + x))) over the items x of the batch whose hash is key i of
 * `t`, w = min(votes(whole), 2047), e = min(votes(forward end) + votes(reverse end), 4095), the votes looked up in vote_table (its
 * counts; a table without counts gives 1).  d_best (one uint64_t per key of t) is the caller's: zeroed before the first batch,
 * carried from batch to batch; a 0 left at the end means no occurrence (every occurrence has w >= 1).  One 64-bit atomicMax per
 * item, the only atomic on an output; max does not depend on the order, so d_best is a function of the input.  The checks of
 * s2k_table_vote_keys apply; ordinal_base + the batch's items > 2^40 is refused on the host; a key that vote_table lacks (it is not
 * the table counted from these batches) is S2K_ERR_INVALID_ARG, found on the device before anything is written.  Workspace: 12.2 B
 * per item and 1 B per base.  Runs on t's context's stream; returns when d_best is written. */
s2k_status s2k_table_vote_representatives(s2k_table *t, s2k_table *vote_table, uint64_t n_reads, const s2k_device_out *in, uint32_t k,
                                          const uint8_t *d_bases, const uint64_t *d_read_off, uint64_t ordinal_base, uint64_t *d_best);
/* d_rep[i] = 2^40 - 1 - (d_best[i] & (2^40 - 1)), or all ones where d_best[i] == 0: the d_rep that s2k_table_node_sequences takes. */
s2k_status s2k_vote_ordinals(s2k_ctx *ctx, const uint64_t *d_best, uint64_t n, uint64_t *d_rep);
/* ---- read walks aligned to their paths: targets, edit distance and CIGAR ----------------------------------------------
 * Targets.  Inputs: the walk records first_step, n_steps, path_start, path_end and flags that s2k_paths_walks wrote (n_walks of each),
 * the oriented unitig of every step of the paths (d_step_unitig, n_steps entries), and d_out_off, d_out (n_bases bytes) and d_overlap of
 * s2k_unitig_sequences over n_unitigs unitigs.  Step j of a walk runs on U_j = step_unitig[first_step + j]; its string s_j is the
 * unitig's bases for an even U_j and revcomp of them (above) for an odd one, L_j its length.  The stitched path is s_0 followed by
 * s_j[overlap[U_(j-1)]:] for j = 1 .. n_steps - 1; target w is its bytes [path_start, path_end).  For a walk with S2K_WALK_CIRCULAR
 * (one step) byte x of the target is s_0[x mod L_0]: path_end may pass L_0, more than once.
 * A walk is bad, which is no error of the call, when a junction has overlap[U_(j-1)] > min(L_(j-1), L_j) (representatives of
 * erroneous reads can give one), when it is circular with L_0 == 0 or without a step, when path_start > path_end, or when it is not
 * circular and path_end passes the stitched length.  A bad walk has d_bad[w] = 1 and an empty target; every other walk d_bad[w] = 0.
 * d_tgt_off (n_walks + 1 entries, may be NULL): tgt_off[w + 1] - tgt_off[w] = path_end - path_start, 0 for a bad walk; d_bad (n_walks
 * bytes, may be NULL); d_tgt (may be NULL: the sizes only; 16-byte aligned, stores are 16 bytes wide) the bytes; *n_bytes is always
 * set.  *n_bytes > capacity with d_tgt given is S2K_ERR_CAPACITY and nothing at all is written.  Checked on the device before
 * anything is written, one flag word read by the host, S2K_ERR_INVALID_ARG otherwise: every walk's steps lie inside the n_steps steps;
 * every step's unitig < 2 n_unitigs; out_off does not decrease and ends inside n_bases; no unitig of 2^32 bases or more; no target of
 * 2^32 bytes or more.  n_unitigs >= 2^31 is refused.  d_out is read in aligned 8-byte words (it must be 8-byte aligned and its
 * allocation whole words, as the node pool); the contents of d_overlap are only compared.  Lengths by one lane per walk from two
 * scans over the steps, a scan over the lengths, then an output-ordered copy: consecutive lanes take consecutive 16 bytes, the step
 * of a byte is found by a search of the walk's per-step prefix, a twin strand is complemented in registers.  No atomic on an output:
 * every output is a function of the input.  Workspace (the context's grow-only count workspace): 24 B per step and 13 B per walk.
 * Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_walks_targets(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                             const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps,
                             const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs,
                             uint64_t *d_tgt_off, uint8_t *d_tgt, uint8_t *d_bad, uint64_t capacity, uint64_t *n_bytes);
/* Pairs.  Pair i aligns q = d_query[q_begin[i], q_end[i]) with t = d_target[t_begin[i], t_end[i]) (absolute in their pools of
 * n_query_bytes and n_target_bytes), globally, at unit costs: a mismatch 1, an inserted or deleted base 1.  Bytes are compared as they
 * are: no case folding, N == N.  No load touches a byte outside a pool.
 * The rule, on furthest-reaching points.  m = |q|, n = |t|; diagonal k = j - i for i bases of q and j of t consumed; ext(i, k) = i
 * advanced while i < m, i + k < n and q[i] == t[i + k].  H[0][0] = ext(0, 0).  For s >= 1 and -s <= k <= s the candidates are H[s-1][k]
 * + 1 (X), H[s-1][k+1] + 1 (I: a query base without a target base) and H[s-1][k-1] (D: a target base without a query base), each only
 * where its source exists, and kept only if i <= m and 0 <= i + k <= n; without a candidate H[s][k] does not exist, otherwise v = the
 * largest candidate and H[s][k] = ext(v, k).  edits = the smallest s with H[s][n - m] == m.
 * Traceback from (s = edits, k = n - m, i = m): v = v of (s, k) (0 at s == 0); emit i - v bases of '='; i = v; stop at s == 0;
 * otherwise take the first predecessor that gives v -- X if H[s-1][k] + 1 == v: i -= 1; I if H[s-1][k+1] + 1 == v: i -= 1, k += 1; D
 * (H[s-1][k-1] == v): k -= 1 -- and s -= 1.  The result reversed, equal neighbours merged into runs: at most 2 edits + 1 runs.
 * Outputs per pair: edits; flags, bit 0 S2K_ALIGN_OVER = the distance exceeds max_edits (|n - m| > max_edits decides at once), then
 * edits = max_edits + 1 and n_ops = matches = 0; ops_off (n_pairs + 1 entries) = the exclusive scan of 2 edits + 1 over the pairs
 * that are not over and of 0 over those that are; n_ops; matches = the bases under '='; ops, one uint32_t per run, len << 4 | op with
 * the BAM codes below: the CIGAR of pair i is ops[ops_off[i] .. ops_off[i] + n_ops[i]), the slots behind it are left untouched.
 * A call with out NULL or without ops, n_ops and matches is the sizes call: it writes edits, flags and ops_off (those given) and
 * *n_ops_bound = ops_off[n_pairs], which is always set.  A call with one of ops, n_ops, matches needs edits, flags and ops_off too (the
 * second pass reads edits and ops_off back), and out->capacity, in runs: *n_ops_bound > capacity is S2K_ERR_CAPACITY and nothing at all is written.
 * S2K_ERR_INVALID_ARG, nothing written (found on the device, one flag word read by the host): a begin above its end, an interval
 * outside its pool, an interval of 2^31 bytes or more; on the host: max_edits > S2K_ALIGN_MAX_EDITS, n_pairs >= 2^32.  n_pairs == 0
 * reads nothing.  S2K_ALIGN_BAD_PATH is never set here: it marks, in the flags a caller keeps per walk, a walk whose target
 * s2k_walks_targets called bad.
 * One wave per pair, lanes across the diagonals of a wavefront; a bounded grid of at most S2K_ALIGN_WAVES waves in which a wave takes
 * the next pair off a counter in the workspace.  Two passes: the distances with two wavefronts in registers and no storage, then,
 * ops_off known, the wavefronts again with every H kept, and the traceback, which recomputes v.  No atomic touches an output and which
 * wave took a pair reaches none: two calls are bit-identical.  Workspace (the context's grow-only count workspace): 20 B per pair,
 * then 4 (emax + 1)^2 B per wave in flight, emax = the largest distance of a pair that is not over (<= max_edits), over min(n_pairs,
 * S2K_ALIGN_WAVES) waves, fewer (never below 4) where that would pass 256 MiB.  Runs on the context's stream; returns when the outputs
 * are written. */
#define S2K_ALIGN_OVER 1u
#define S2K_ALIGN_BAD_PATH 2u
#define S2K_ALIGN_MAX_EDITS 255u
#define S2K_ALIGN_WAVES 2048u
#define S2K_CIGAR_I 1u
#define S2K_CIGAR_D 2u
#define S2K_CIGAR_EQ 7u
#define S2K_CIGAR_X 8u
typedef struct s2k_align_out { /* device pointers, each may be NULL; capacity in runs */
    uint64_t capacity;
    uint32_t *edits;
    uint32_t *flags;
    uint64_t *ops_off; /* n_pairs + 1 */
    uint32_t *n_ops;
    uint32_t *matches;
    uint32_t *ops;
} s2k_align_out;
s2k_status s2k_align_pairs(s2k_ctx *ctx, const uint8_t *d_query, uint64_t n_query_bytes, const uint8_t *d_target, uint64_t n_target_bytes,
                           const uint64_t *d_q_begin, const uint64_t *d_q_end, const uint64_t *d_t_begin, const uint64_t *d_t_end, uint64_t n_pairs,
                           uint32_t max_edits, const s2k_align_out *out, uint64_t *n_ops_bound);
/* ---- pile-up and consensus: the aligned walks vote on the unitigs' bases ---------------------------------------------
 * Pile-up.  Inputs: the walk records, d_step_unitig, d_out_off, d_out (n_bases bytes), d_overlap and n_unitigs exactly as
 * s2k_walks_targets takes them; the query pool d_query (n_query_bytes) and per walk d_q_begin, where its query interval starts; per walk
 * the alignment's d_align_flags, d_ops_off (n_walks + 1), d_n_ops, and d_ops (n_ops_total runs, len << 4 | op) as s2k_align_pairs wrote
 * them for the pairs (query interval, target of the walk); max_shift <= S2K_PILEUP_MAX_SHIFT.
 * The pile (s2k_pile, device pointers, the caller's): eleven planes of n_bases uint32_t each, indexed by position in d_out, the forward
 * strand of the unitig: match, del, sub[4], ins[4], ins_long -- 44 B per base, plain counts.  Zeroed before the first batch and carried
 * from batch to batch and from file to file, as d_best above.  The pile is a function of the multiset of walks, whatever the batch cut.
 * Which walks vote: a walk with d_align_flags[w] != 0 (S2K_ALIGN_OVER, S2K_ALIGN_BAD_PATH) votes nothing and is counted; every other
 * walk votes by the rule below.  A walk that s2k_walks_targets calls bad has an empty target here too.
 * Source of a target byte: byte x of walk w's target comes from the step j and the offset o in s_j from which s2k_walks_targets copies
 * it: overlapped bytes belong to the earlier step; on a circular walk o = (path_start + x) mod L, and a round (path_start + x) / L
 * counts as a step of its own below.  Its forward position is p = out_off[t] + o on an even unitig and out_off[t] + L - 1 - o on an odd
 * one.  A query byte that votes on an odd step is complemented.  Codes: A/a 0, C/c 1, G/g 2, T/t 3; an X byte without a code casts no
 * vote and is counted (n_other).
 * Pieces: runs of =, X and D are cut where the step of the target byte changes; each piece covers a forward interval [a, b) of one
 * unitig.  An I run of n bytes between target bytes x - 1 and x belongs to the step of byte x - 1 (of byte 0 at x == 0; with an empty
 * target it is dropped and counted, n_empty_ins); its forward gap g, the position it is inserted before, is p(x - 1) + 1 on an even step
 * (p(0) at x == 0) and p(x - 1) on an odd one (p(0) + 1 at x == 0).
 * Normalisation: gaps are left-aligned on the forward strand.  The forward-left neighbour of a gap run (I or D) is the run before it in
 * the CIGAR on an even step and the run behind it on an odd one.  The shift d is 0 unless that neighbour is =, the gap run is one piece,
 * and the neighbour's piece next to the gap lies in the same step, e its length; then d is the largest d <= min(e, max_shift) with, for
 * i = 1 .. d, out[a - i] == out[b - i] for D, and out[g - i] == c[n - 1 - ((i - 1) mod n)] for I, c the inserted bytes in forward
 * orientation (reversed and complemented on an odd step); bytes are compared as they are.
 * Votes: D: del += 1 over [a - d, b - d), and the neighbouring = piece votes match += 1 over its interval without [a - d, a) and with
 * [b - d, b) in its place; every other = piece match += 1 over its interval; X: sub[code][p] += 1 per byte; an I run of one byte with
 * a code: ins[code][g - d] += 1; any other I run: ins_long[g - d] += 1 (an I shift leaves match as it was); a gap at g - d == the
 * unitig's end is dropped and counted (n_end_ins).
 * stats (host, S2K_PILEUP_STATS words, always set, zeros on a refusal): walks used, walks skipped, n_other, n_end_ins, gaps shifted,
 * n_empty_ins, 0, 0.
 * Checked on the device before anything is written, S2K_ERR_INVALID_ARG and nothing written otherwise (flag words read by the host):
 * the checks of s2k_walks_targets; ops_off does not decrease and ends inside n_ops_total, n_ops[w] <= ops_off[w + 1] - ops_off[w];
 * every run of a voting walk has a known code and a length above 0; the runs of a voting walk consume exactly its target's length; its
 * query interval [q_begin, q_begin + the query bytes of its runs) lies inside the pool.  On the host: max_shift above
 * S2K_PILEUP_MAX_SHIFT, a plane that is NULL, n_walks >= 2^32.
 * One lane per run slot; a run's offsets in target and query are differences of two scans over all slots; no lane walks a match run:
 * = and D pieces add +1 / -1 at their ends to two difference planes in the workspace, which a scan each adds into match and del; X
 * bytes and I runs are one 32-bit atomic add each.  Integer sums are the only atomics on an output: two calls on equal piles give
 * equal piles.  Workspace (the context's grow-only count workspace): 24 B per step, 13 B per walk, 28 B per run slot, 16 B per base.
 * Runs on the context's stream; returns when the pile is written.
 * Not done: votes on both copies of an overlapped base (a unitig's head that is entered along an edge is voted only by walks that start
 * in it); quality values; a pile over several devices.  Insertions of two or more bases: s2k_walks_pileup_ex below. */
#define S2K_PILEUP_MAX_SHIFT 64u
#define S2K_PILEUP_STATS 8
#define S2K_CONSENSUS_STATS 8
#define S2K_LONG_INS_MIN 2u  /* the shortest and the longest I run that gets a vote key (s2k_walks_pileup_ex) */
#define S2K_LONG_INS_MAX 12u
#define S2K_LONG_INS_POS_BITS 36 /* a vote key holds this many bits of the position: n_bases < 2^36 */
typedef struct s2k_pile { /* device pointers, n_bases uint32_t each */
    uint32_t *match;
    uint32_t *del;
    uint32_t *sub[4];
    uint32_t *ins[4];
    uint32_t *ins_long;
} s2k_pile;
s2k_status s2k_walks_pileup(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                            const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps, const uint64_t *d_out_off,
                            const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs, const uint8_t *d_query,
                            uint64_t n_query_bytes, const uint64_t *d_q_begin, const uint32_t *d_align_flags, const uint64_t *d_ops_off,
                            const uint32_t *d_n_ops, const uint32_t *d_ops, uint64_t n_ops_total, uint32_t max_shift, const s2k_pile *pile, uint64_t *stats);
/* Pile-up with the vote keys of long insertions.  The arguments, the checks, the pile written (bit for bit, ins_long
 * counts every long run, keyed or not) and the stats words are those of s2k_walks_pileup.
 * A keyed run is an I run of a voting walk of S2K_LONG_INS_MIN <= n <= S2K_LONG_INS_MAX bytes, every byte with a code, that the rule
 * above neither drops (n_empty_ins, n_end_ins) nor skips.  With g, d and c (the inserted bytes in forward orientation) as above, the
 * run is inserted before forward position at = g - d and reads there s[i] = c[(i - d) mod n], i = 0 .. n - 1 (c rotated right by
 * d mod n).  Its key is
 *     rev36(at) << 28 | n << 24 | sum_i code(s[i]) << (22 - 2 i)
 * rev36 the reversal of the low 36 bits of at; unused code bits 0; codes on the forward strand.  All candidates of one position are
 * one range of a sorted table; the reversed position spreads the top digits of the counter's radix partition; n is never 15, so no
 * key is the counter's empty value 2^64 - 1.  The keys go to an s2k_counter (s2k_counter_add) batch by batch; the multiset of keys is
 * a function of the multiset of walks, whatever the batch cut.
 * *n_candidates (host, always set; 0 on a refusal by a check): the I runs of voting walks with 2 <= n <= 12, known from the run slots
 * before anything is written.  d_long_keys NULL: no keys, *n_long_keys = 0.  d_long_keys given and capacity < *n_candidates:
 * S2K_ERR_CAPACITY and nothing at all is written, the pile included.  Otherwise the keys of the keyed runs stand compact in
 * d_long_keys[0 .. *n_long_keys), in run-slot order: a flag per run slot and a scan, no atomic cursor; two calls are bit-identical.
 * S2K_ERR_INVALID_ARG on the host, before any launch: d_long_keys given with n_bases >= 2^36; n_candidates or n_long_keys NULL.
 * One lane per run; the lane of a keyed run reads its at most 12 bytes.  Workspace: with d_long_keys 12 B more per run slot (flag, key).
 * Not keyed, counted in ins_long only: runs above 12 bytes or with a byte without a code.  Not done: an insertion that the aligner
 * split into two I runs is not merged. */
s2k_status s2k_walks_pileup_ex(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_first_step, const uint32_t *d_n_steps, const uint64_t *d_path_start,
                               const uint64_t *d_path_end, const uint32_t *d_flags, const uint32_t *d_step_unitig, uint64_t n_steps,
                               const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases, const uint32_t *d_overlap, uint64_t n_unitigs,
                               const uint8_t *d_query, uint64_t n_query_bytes, const uint64_t *d_q_begin, const uint32_t *d_align_flags,
                               const uint64_t *d_ops_off, const uint32_t *d_n_ops, const uint32_t *d_ops, uint64_t n_ops_total, uint32_t max_shift,
                               const s2k_pile *pile, uint64_t *stats, uint64_t *d_long_keys, uint64_t capacity, uint64_t *n_candidates,
                               uint64_t *n_long_keys);
/* Consensus, once per graph; the pile is only read, so more batches may be added afterwards.  Per position p of a unitig, cur = the code
 * of out[p] (none for another byte): tot[c] = sub[c][p] + (c == cur ? match[p] : 0); for a byte without a code match[p] counts for
 * the byte itself as a fifth candidate; depth = match + the four sub + del.  depth < min_cov: the byte is kept, nothing is inserted,
 * n_low counts it.  Otherwise, first the insertion before p: best = the code with the largest ins[c][p], the smallest among equals; if
 * 2 ins[best][p] > depth the letter ACGT[best] is emitted (n_ins).  Then the base: if del[p] is strictly above every candidate nothing
 * is emitted (n_del); otherwise, if the current byte's count equals the largest, the byte is kept as it is, case included; otherwise
 * the upper-case letter of the smallest code with the largest count is emitted (n_sub).  A position with 2 ins_long[p] > depth is
 * counted (n_long) and otherwise left alone (s2k_pileup_consensus_ex below calls it).
 * Outputs (each may be NULL): d_new_out_off (n_unitigs + 1); d_new_out (16-byte aligned; capacity in bytes; for s2k_walks_targets to
 * read it its allocation must be whole 8-byte words, as d_out's); d_pos_map (n_bases + 1): the new position of every old one, an
 * inserted letter belongs to the position it precedes, pos_map[n_bases] = *n_new_bases; d_new_overlap (2 n_unitigs): with ov' =
 * min(overlap[U], L) and pm relative to the unitig, newL - pm(L - ov') for an even U and pm(ov') for an odd one.  *n_new_bases is always
 * set; d_new_out NULL is the sizes call (the other outputs given are written); *n_new_bases > capacity with d_new_out given is
 * S2K_ERR_CAPACITY and nothing at all is written.  stats (host, S2K_CONSENSUS_STATS words): n_low, n_sub, n_del, n_ins, n_long, 0, 0,
 * 0; zeros on a refusal.  S2K_ERR_INVALID_ARG, nothing written: out_off that decreases or passes n_bases, a unitig of 2^31 bases or
 * more (found on the device); a NULL plane, d_new_out not 16-byte aligned (on the host).  Positions outside [out_off[0],
 * out_off[n_unitigs]) emit nothing.
 * One lane per position decides its 0 to 2 bytes, one scan gives pos_map, then input-ordered stores: lane p writes its bytes at
 * pos_map[p].  No atomic on an output: two calls are bit-identical.  Workspace: 14 B per base.  Runs on the context's stream; returns
 * when the outputs are written.
 * Not done: a second round on the polished coordinates (walks and member offsets are not remapped). */
s2k_status s2k_pileup_consensus(s2k_ctx *ctx, const s2k_pile *pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases,
                                const uint32_t *d_overlap, uint64_t n_unitigs, uint32_t min_cov, uint64_t *d_new_out_off, uint8_t *d_new_out,
                                uint64_t capacity, uint64_t *d_pos_map, uint32_t *d_new_overlap, uint64_t *n_new_bases, uint64_t *stats);
/* Consensus that calls insertions of two or more bases from a table of vote keys: d_long_keys (strictly ascending) and
 * d_long_counts, n_long_keys of each, as s2k_counter_finish writes them for the keys of s2k_walks_pileup_ex.  With n_long_keys == 0 it
 * is s2k_pileup_consensus in every output and every stats word.  Otherwise, at a position p with depth >= min_cov, the insertion before
 * p: cs = the count of the best single letter as above; the candidates of p are the entries with key >> 28 == rev36(p); L the candidate
 * with the largest count, the smallest key among equals, cl its count (0 without a candidate).  cl > cs and 2 cl > depth: the n
 * upper-case letters of L are emitted, stats[5] (n_ins_long) counts the position and stats[6] (n_ins_long_bases) gains n.  Otherwise, if
 * 2 cs > depth, the single letter as above.  The base at p is decided as above.  n_long counts the positions with 2 ins_long[p] > depth
 * at which no long insertion was called.  The counts are trusted; a lane searches the table only where 2 ins_long[p] > depth (cl <=
 * ins_long[p]).  pos_map, new_out_off and new_overlap keep their definitions: inserted letters belong to the position they precede.
 * Checked on the device before anything is written, S2K_ERR_INVALID_ARG otherwise: keys strictly ascending, every n field in
 * S2K_LONG_INS_MIN .. S2K_LONG_INS_MAX.  On the host: a table with n_bases >= 2^36 or of 2^32 - 1 keys or more, a NULL table array.
 * A position emits 0 to 13 bytes: the call leaves the candidate's index per position, the input-ordered write decodes its letters from
 * the key.  Workspace: 18 B per base with a table, 14 B without. */
s2k_status s2k_pileup_consensus_ex(s2k_ctx *ctx, const s2k_pile *pile, const uint64_t *d_out_off, const uint8_t *d_out, uint64_t n_bases,
                                   const uint32_t *d_overlap, uint64_t n_unitigs, uint32_t min_cov, uint64_t *d_new_out_off, uint8_t *d_new_out,
                                   uint64_t capacity, uint64_t *d_pos_map, uint32_t *d_new_overlap, uint64_t *n_new_bases, uint64_t *stats,
                                   const uint64_t *d_long_keys, const uint32_t *d_long_counts, uint64_t n_long_keys);
/* ---- segmented alignment: long walks cut at anchor k-min-mers, aligned piece by piece, joined --------------------------
 * s2k_align_pairs aligns at most S2K_ALIGN_MAX_EDITS edits per pair, and a walk of a long noisy read passes that.  Every solid item of
 * a threaded step is an exact anchor between the read and the walk's stitched path; s2k_walks_segments cuts a walk at a thinned,
 * strictly increasing subset of them into segment pairs that s2k_align_pairs takes as they are, and s2k_align_join puts the segments'
 * CIGARs back together, one alignment per walk, in the layout s2k_walks_pileup and the GAF writer take.
 * Inputs of s2k_walks_segments.  walks: the records s2k_paths_walks wrote (walk_off over n_reads reads, first_step, n_steps, qstart,
 * qend, path_start, path_end, flags; n_walks of each; the other fields are not read); paths: unitig, pos and count of the n_steps steps
 * the walks were made on (path_off is not read); the decomposition and where its members lie in base space exactly as
 * s2k_paths_walks takes them (d_uni_off, d_members, d_circular, d_member_off, d_out_off, d_overlap, d_seq_len; n_unitigs, n_nodes); per
 * walk d_q_begin, where its query interval starts in the batch's bases (as s2k_walks_pileup takes it), and d_tgt_off (n_walks + 1) and
 * d_bad as s2k_walks_targets wrote them; src: the SOURCE paths, what s2k_table_thread wrote for the same reads (path_off, pos, count
 * and item are required; n_src_steps), on which item i of step r is exactly the read's item item[r] + i at position pos[r] + i of the
 * step's oriented unitig; in: km_off and start of the batch's s2k_device_out.  Two optional maps, one entry per source step:
 * d_src_step[r], the step of `paths` that source step r went into, S2K_NO_STEP for none (NULL: the identity, the walks were made on src
 * itself), and d_src_pos[r], the position of r's first item on that step's oriented unitig (NULL: src->pos).  s2k_paths_bridge keeps
 * unitig and position, so after it src_step[r] = (the source steps r' <= r with join[r'] != 1) - 1 and src_pos = src->pos.  seg_len, in
 * bases: 0 means S2K_SEGMENT_LEN; a value below S2K_SEGMENT_MIN_LEN is refused.
 * Candidates, in source-item order (read by read, step by step, item by item).  Item i of source step r of read R is the read's item j
 * = km_off[R] + item[r] + i.  S = src_step[r], w = the walk with first_step[w] <= S < first_step[w] + n_steps[w], x = src_pos[r] + i.
 * The item is OUTSIDE -- counted, never an error -- when S is S2K_NO_STEP, when no walk holds S, when x is not in [pos[S], pos[S] +
 * count[S]) or not below the members of the step's unitig, when walk w has S2K_WALK_CIRCULAR, or when d_bad[w] != 0.  Every other item
 * is a candidate of walk w with, as integers that may be negative,
 *   qc = in->start[j] - qstart[w]                                  (its offset in the walk's query interval) and
 *   tc = G_w[S] + lo(unitig[S], x) - path_start[w]                 (its offset in the walk's target),
 * lo the first base of position x of the oriented unitig exactly as "Base interval of a position" above has it, and G_w[S] the sum of
 * adv(unitig) over the walk's steps before S, adv as for s2k_paths_walks.  Both sides start at the first base of the item's first
 * minimizer, so on an error-free read query byte qc IS target byte tc.
 * Admissible: with m = qend[w] - qstart[w] and n = tgt_off[w + 1] - tgt_off[w], a candidate is admissible iff 0 < qc < m, 0 < tc < n, qc
 * is strictly above the qc of EVERY earlier candidate of the walk (admissible or not) and tc strictly above the tc of every earlier
 * candidate of the walk.  Admissible anchors of a walk therefore increase strictly in both coordinates, whatever the representatives
 * of erroneous reads did to the member offsets.
 * Chosen: an admissible candidate is chosen iff qc / seg_len >= 1 and the admissible candidate of the same walk before it, if there is
 * one, has another qc / seg_len (integer division): the first admissible anchor of every bucket of seg_len query bases but the first.
 * Segments: a walk with a chosen anchors gives a + 1 segments between the cuts (0, 0), the chosen (qc, tc) in order, (m, n): segment
 * k is query [q_begin[w] + qc_k, q_begin[w] + qc_(k+1)) against target [tgt_off[w] + tc_k, tgt_off[w] + tc_(k+1)).  A circular walk
 * and a walk without a chosen anchor give one segment, the whole pair; a bad walk one segment that is empty on both sides, at
 * (q_begin[w], tgt_off[w]).  Every walk has at least one segment; a cut walk's segments are non-empty on both sides.
 * s2k_segment_out (device pointers, each may be NULL; capacity in segments): seg_off (n_walks + 1): the segments of walk w are
 * [seg_off[w], seg_off[w + 1]); q_begin, q_end, t_begin, t_end, one uint64_t per segment, absolute in the two pools: they go to
 * s2k_align_pairs unchanged.  *n_segments is always set.  stats (host, S2K_SEGMENT_STATS words, always set, zeros on a refusal):
 * candidates, outside, admissible, chosen, walks cut at least once, 0, 0, 0.  out NULL or without the four interval arrays asks for the
 * sizes (seg_off, when given, is written whenever the call returns S2K_OK); *n_segments > out->capacity with an interval array given
 * is S2K_ERR_CAPACITY and nothing at all is written.
 * Checked on the device before anything is written, flag words read by the host, S2K_ERR_INVALID_ARG otherwise: the checks of
 * s2k_walks_targets on the walks and the steps' unitigs (every walk's steps inside the paths, every unitig < 2 n_unitigs, out_off not
 * decreasing, no unitig of 2^32 bases or more) and those of s2k_paths_walks on the steps and the decomposition (count >= 1, pos < len,
 * pos + count <= len unless the unitig is circular; uni_off strictly ascending from 0 to n_nodes; every member < 2 n_nodes; every
 * member_off inside its unitig's bases); walk_off and src->path_off run from 0 to n_walks and to n_src_steps without decreasing; the
 * walks' step ranges ascend without overlapping (first_step[w] + n_steps[w] <= first_step[w + 1]); qstart <= qend; tgt_off does not
 * decrease and no target has 2^32 bytes or more; km_off does not decrease and km_off[R] + item[r] + count[r] <= km_off[R + 1];
 * src_step[r] is below n_steps or S2K_NO_STEP; the walk that holds src_step[r] is a walk of r's read; src_step does not decrease from
 * a source step to the next one of its read where both have a step, nor does the walk of a candidate lie before the walk of an
 * earlier one.  On the host: seg_len below S2K_SEGMENT_MIN_LEN, n_unitigs or n_nodes or n_walks >= 2^31.  d_seq_len, d_q_begin and the
 * contents of d_overlap and d_bad are trusted, and in->start is trusted to hold km_off[n_reads] entries.
 * One lane per source step, then one lane per item: the two "strictly above" tests are exclusive max-scans over all items of the
 * batch (a walk's index in the high half of the scanned word keeps the walks apart: walks come in read order), the admissible
 * anchors are compacted, the chosen ones are the heads of a mask over the compacted stream and are compacted again, seg_off is a
 * search per walk and the intervals are written one lane per segment.  No lane walks a walk.  The counters are integer sums and no
 * atomic touches an output: two calls are bit-identical.  Workspace (the context's grow-only count workspace): 28 B per item (two
 * scanned words, three compacted words) and twice 12 B per 64 items and 12 B per tile of 2 048 for the masks; 20 B per source step;
 * 16 B per step of the paths; 8 B per walk.  Runs on the context's stream; returns when the outputs are written.
 * Not done: the map through s2k_paths_lift (ContigLift.lift) is not composed anywhere: d_src_step / d_src_pos carry it, nothing
 * computes them, and until then walks on lifted paths are aligned whole (s2k_align_pairs); re-anchoring (an anchor is never searched
 * for, moved or verified against the bases); choosing among walks; affine gaps; a globally optimal score -- the joined alignment is
 * a valid alignment of the walk, optimal between its cuts only. */
#define S2K_NO_STEP 0xFFFFFFFFFFFFFFFFull
#define S2K_SEGMENT_LEN 512u
#define S2K_SEGMENT_MIN_LEN 64u
#define S2K_SEGMENT_STATS 8
typedef struct s2k_segment_out { /* device pointers, each may be NULL; capacity in segments */
    uint64_t capacity;
    uint64_t *seg_off; /* n_walks + 1 */
    uint64_t *q_begin;
    uint64_t *q_end;
    uint64_t *t_begin;
    uint64_t *t_end;
} s2k_segment_out;
s2k_status s2k_walks_segments(s2k_ctx *ctx, uint64_t n_reads, const s2k_walk_out *walks, uint64_t n_walks, const s2k_thread_out *paths,
                              uint64_t n_steps, const uint64_t *d_uni_off, const uint32_t *d_members, const uint8_t *d_circular,
                              uint64_t n_unitigs, const uint64_t *d_member_off, const uint64_t *d_out_off, const uint32_t *d_overlap,
                              const uint32_t *d_seq_len, uint64_t n_nodes, const uint64_t *d_q_begin, const uint64_t *d_tgt_off,
                              const uint8_t *d_bad, const s2k_thread_out *src, uint64_t n_src_steps, const uint64_t *d_src_step,
                              const uint32_t *d_src_pos, const s2k_device_out *in, uint32_t seg_len, const s2k_segment_out *out,
                              uint64_t *n_segments, uint64_t *stats);
/* Join.  Inputs: d_seg_off (n_walks + 1) and d_bad (one byte per walk) as above, and seg, the arrays s2k_align_pairs wrote for the
 * n_segments segment pairs (edits, flags, ops_off, n_ops, matches, ops; seg->capacity = the runs ops holds).  Output: `out`, one
 * alignment per walk in the layout of s2k_align_pairs, but compact: ops_off (n_walks + 1) is the exclusive scan of the joined n_ops.
 * A bad walk (d_bad[w] != 0) gets flags = S2K_ALIGN_BAD_PATH and edits = n_ops = matches = 0.  Otherwise a walk with a segment that
 * has S2K_ALIGN_OVER gets flags = S2K_ALIGN_OVER, n_ops = matches = 0 and edits = the sum over its segments, a lower bound (an over
 * segment counts max_edits + 1).  Every other walk gets flags = 0, edits and matches = the sums over its segments, and as its CIGAR the
 * segments' runs in order, where the first run of a segment after the walk's first is merged into the run before it when the segment
 * before it has a run and that segment's last run has the same op; a chain of all-'=' segments thus becomes one run.  A run is a HEAD
 * unless it is so merged; n_ops = the heads of the walk, and a head's length is the sum of its run and the merged runs behind it.
 * *n_ops_total = ops_off[n_walks] is always set.  out NULL asks for the sizes; *n_ops_total > out->capacity with out->ops given is
 * S2K_ERR_CAPACITY and nothing at all is written; otherwise every array of `out` that is given is written.  Checked on the device
 * before anything is written (S2K_ERR_INVALID_ARG): seg_off runs from 0 to n_segments without decreasing; the segments' ops_off does not
 * decrease and ends inside seg->capacity, n_ops[s] <= ops_off[s + 1] - ops_off[s]; every run of a walk that is neither bad nor over has
 * a known code and a length above 0; no merged run has 2^28 bases or more (the length field is 28 bits); no walk's edits or matches
 * sum to 2^32 or more.  On the host: n_walks or n_segments >= 2^32.
 * One lane per run slot of the segments: its segment and walk by searches of the two offset arrays, one head mask, one compaction;
 * merged lengths are differences of a prefix over the slots' lengths taken at consecutive heads, the sums differences of prefixes over
 * the segments; the writes are ordered by output position.  No atomic on an output: two calls are bit-identical.  Workspace: 24 B per
 * run slot (length and prefix; prefix and op of the joined runs, sized by the slots), the mask's 12 B per 64 slots and per tile, 28 B
 * per segment.  Runs on the context's stream; returns
 * when the outputs are written. */
s2k_status s2k_align_join(s2k_ctx *ctx, uint64_t n_walks, const uint64_t *d_seg_off, const uint8_t *d_bad, uint64_t n_segments,
                          const s2k_align_out *seg, const s2k_align_out *out, uint64_t *n_ops_total);
/* ---- GAF text on the device: one line per walk -----------------------------------------------------------------------
 * Inputs: the walk records s2k_paths_walks wrote (walk_off, first_step, n_steps, items, qstart, qend, path_len, path_start, path_end;
 * flags and edge are not read) for n_reads reads and n_walks walks; d_step_unitig, the oriented unitig of every one of the n_steps
 * steps; optionally the reads' names, d_names (n_name_bytes bytes) and d_name_off (n_reads + 1 entries: the name of read r is
 * d_names[name_off[r], name_off[r + 1])), both NULL or both given; first_read; optionally d_read_len (n_reads entries); optionally al,
 * the alignments of the walks as s2k_align_pairs or s2k_align_join wrote them (edits, flags, ops_off, n_ops, matches, ops;
 * al->capacity = the runs ops holds).
 * The line of walk w of read r, fields separated by tabs, unsigned decimal numbers without padding:
 *   name (the bytes as they are, or the decimal first_read + r), the read's length (or *), qstart, qend, +, the path -- per step s in
 *   [first_step, first_step + n_steps) the token >t for d_step_unitig[s] = 2 t and <t for 2 t + 1 --, path_len, path_start, path_end,
 *   matches, block, 255, km:i:<items>, ns:i:<n_steps>, and a newline.  Without al, or with al->flags[w] != 0, matches = items and block =
 *   max(qend - qstart, path_end - path_start).  With al->flags[w] == 0, matches = al->matches[w], block = the sum of the lengths of the
 *   walk's runs ops[ops_off[w] .. ops_off[w] + n_ops[w]), and \tNM:i:<edits>\tcg:Z:<runs> stands before the newline, a run len << 4 | op
 *   as <len> and I, D, =, X for S2K_CIGAR_I, _D, _EQ, _X; n_ops[w] == 0 gives an empty cg:Z:.  The slots behind a walk's n_ops, which
 *   s2k_align_pairs leaves untouched, and every slot of a flagged walk are never read.  Walks may share steps and stand in any order.
 * Outputs: *n_bytes = the bytes of all lines, always set (0 on a refusal); d_line_off (n_walks + 1 entries, may be NULL): line_off[w] =
 * the first byte of walk w's line, line_off[n_walks] = *n_bytes, written whenever the call returns S2K_OK; d_text (may be NULL: the sizes
 * only): the lines back to back in walk order, written only when *n_bytes <= capacity, otherwise S2K_ERR_CAPACITY and nothing at all is
 * written.  n_walks == 0 reads no input and writes line_off[0] = 0 alone.  Outputs must not overlap inputs.
 * Checked on the device before anything is written, one flag word read by the host, S2K_ERR_INVALID_ARG otherwise: walk_off runs from 0
 * to n_walks without decreasing; every walk's steps lie inside the n_steps steps; qstart <= qend and path_start <= path_end; name_off
 * runs from 0 without decreasing and ends inside n_name_bytes; with al: ops_off does not decrease and ends inside al->capacity, ops_off[w]
 * + n_ops[w] <= al->capacity, n_ops[w] <= ops_off[w + 1] - ops_off[w] for a walk with flags 0, and every run of such a walk has one of
 * the four codes (a length of 0 is printed as it is); no line has 2^32 bytes or more.  On the host: names without offsets or offsets
 * without names; n_walks >= 2^31; walks without reads; n_reads, n_steps, al->capacity or the sum of the walks' n_steps >= 2^39;
 * first_read + n_reads past 2^64.
 * Lengths first, bytes second: one lane per step (its token's length), per run slot (whether it is live, its token's length, its run
 * length) and per walk (the line's length from the digits of its fields and differences of the two prefixes), a scan for line_off, one
 * host wait; then one lane per walk (the fields), per path token and per live run slot (its token, at the place the prefixes give).
 * No lane loops over a walk (only over its own digits or a name's bytes: a very long name is slow, never wrong).  No atomic touches
 * an output: two calls are bit-identical.  Workspace (the context's grow-only count workspace): 12 B per step, 24 B per run slot, 28 B
 * per walk.  Runs on the context's stream; returns when the outputs are written. */
s2k_status s2k_walks_gaf(s2k_ctx *ctx, uint64_t n_reads, const s2k_walk_out *walks, uint64_t n_walks, const uint32_t *d_step_unitig,
                         uint64_t n_steps, const uint8_t *d_names, const uint64_t *d_name_off, uint64_t n_name_bytes, uint64_t first_read,
                         const uint64_t *d_read_len, const s2k_align_out *al, uint8_t *d_text, uint64_t capacity, uint64_t *d_line_off,
                         uint64_t *n_bytes);
/* Send buffers of the multi-GPU version: d_out = the keys grouped into n_parts ranges of the hash space (part p holds the
 * hashes h with floor(h * n_parts / 2^64) == p, i.e. split by hash prefix), d_part_off[n_parts + 1] = group starts.  After
 * an all-to-all of the groups, rank p owns every occurrence of its range and counts locally. */
#define S2K_MAX_PARTS 64
s2k_status s2k_partition_device(s2k_ctx *ctx, const uint64_t *d_hash, uint64_t n, uint32_t n_parts, uint64_t *d_out,
                                uint64_t *d_part_off);

/* ---- helpers for device-resident benchmarking ------------------------------------------------- */
/* Fills d_bases[0..n) with the deterministic synthetic ACGT stream (splitmix64 keyed by seed and
 * absolute base index; same function as oracle/s2k_oracle.c:s2k_oracle_synth_bases). */
s2k_status s2k_synth_bases_device(s2k_ctx *ctx, uint64_t seed, uint64_t first_base, uint64_t n, uint8_t *d_bases);
/* HiFi-like synthetic reads (BASELINE configs[3]: lengths ~N(15 000, 2 000), homopolymer runs of geometric length with mean 2,
 * ~0.1 % of them stretched to 20..2999 bases; splitmix64 keyed by (seed, read index); same functions as the oracle's
 * s2k_oracle_hifi_len / s2k_oracle_hifi_read).  s2k_synth_hifi_lengths fills a HOST array with the lengths of reads
 * r0 .. r0+n_reads-1; s2k_synth_hifi_device writes read r0+i at d_bases + d_read_off[i] (d_read_off: device, n_reads+1 entries,
 * the prefix sums of those lengths). */
void s2k_synth_hifi_lengths(uint64_t seed, uint64_t r0, uint64_t n_reads, uint64_t *lengths);
s2k_status s2k_synth_hifi_device(s2k_ctx *ctx, uint64_t seed, uint64_t r0, uint64_t n_reads, const uint64_t *d_read_off, uint8_t *d_bases);
/* Duration in ms of the kernels of the last s2k_extract_device call, measured with HIP events on the
 * context's stream: which: 0 = whole pipeline (first kernel's start to the last one's end), 1 = the minimizer kernel (dominant; the
 * descriptor path launches it once per chunk of tiles: first start to last end), 2 = scan + k-min-mer kernels (first start to last
 * end; on the descriptor path they run on a second stream BESIDE the minimizer kernel of the next chunk, so 1 and 2 overlap and
 * do not add up to 0). */
s2k_status s2k_last_kernel_ms(s2k_ctx *ctx, int which, float *ms);
s2k_status s2k_enable_timing(s2k_ctx *ctx, int on);
/* Sum over every s2k_extract_device call since s2k_enable_timing(ctx, 1) of the same HIP-event
 * durations (`which` as above), and the number of calls: average kernel duration over a timed region. */
s2k_status s2k_timing_total(s2k_ctx *ctx, int which, double *ms_sum, uint32_t *n_calls);

/* ---- FASTA / FASTQ ingest and batching (next row of SURVEY.md 8f) --------------------------------------
 * Counterpart of the reference's file mode: rust_parallelfastx::parallel_fastx(file, threads, task) feeding one
 * KminmersIterator per record (src/main.rs:51-83).  Records are parsed on the host into batches
 * (bases back to back + read_off) held in pinned memory, so a batch is what s2k_extract consumes. */
typedef struct s2k_fastx s2k_fastx; /* opaque reader */
/* Opens a plain (uncompressed) FASTA (multi-line allowed) or FASTQ (4-line) file; the format is detected from the
 * first non-blank byte. */
s2k_fastx *s2k_fastx_open(const char *path, s2k_status *status);
/* Parses the next records until `max_bases` bases or `max_reads` reads are collected (at least one record).
 * *bases / *read_off point into reader-owned buffers, valid until the next call; *n_reads == 0 at end of file. */
s2k_status s2k_fastx_next(s2k_fastx *rd, uint64_t max_bases, uint64_t max_reads, const uint8_t **bases,
                          const uint64_t **read_off, uint64_t *n_reads);
void s2k_fastx_close(s2k_fastx *rd);
/* Record splitting on the GPU: FASTA/FASTQ text that is already in HBM (d_text, 16-byte aligned, < 4 GiB, beginning
 * at a record start and ending at a record end) becomes the (bases, read_off) pair s2k_extract_device consumes.
 * format: S2K_FASTA (multi-line allowed) or S2K_FASTQ (strict 4-line records).  *n_reads / *n_bases always receive
 * the sizes; S2K_ERR_CAPACITY when bases_capacity < *n_bases or off_capacity < *n_reads + 1 (call again),
 * S2K_ERR_INVALID_ARG for malformed text.  FASTQ is rejected when a header line does not start with '@' or a third line
 * not with '+', when the text ends inside a record (after a header, a sequence or a '+' line), and when a blank line
 * stands before the first record, between two records or in place of a '+' line; blank lines behind the last record
 * are accepted.  (s2k_fastx_open / s2k_fastx_next skip blank lines before and between records; s2k_run_file skips
 * those before the first record and is as strict as this call about the rest.) */
enum { S2K_FASTA = 0, S2K_FASTQ = 1 };
s2k_status s2k_fastx_parse_device(s2k_ctx *ctx, const uint8_t *d_text, uint64_t n_bytes, int format, uint8_t *d_bases,
                                  uint64_t bases_capacity, uint64_t *d_read_off, uint64_t off_capacity,
                                  uint64_t *n_reads, uint64_t *n_bases);
/* Streams a whole file through the GPU in batches of ~batch_bases and returns the totals: the file's bytes are
 * staged to HBM by several threads, records are split on the GPU (as s2k_fastx_parse_device), and staging +
 * splitting of batch i+1 overlap the k-min-mer kernels of batch i; k-min-mers are produced in HBM and counted, like the reference's demo task
 * (src/main.rs:65-76).  `seconds` receives the wall time of the whole call (file read included). */
s2k_status s2k_run_file(s2k_ctx *ctx, const char *path, const s2k_params *params, uint64_t batch_bases,
                        s2k_counts *totals, double *seconds);
/* s2k_run_file that also counts: the k-min-mer hashes of every batch are added to `counter` (s2k_counter_add) before the batch's
 * buffers are reused; totals and seconds as s2k_run_file (seconds include the counting).  Call it on several files with one counter
 * to count a multi-file dataset, then s2k_counter_finish.  The counter's context must be on ctx's device (S2K_ERR_INVALID_ARG). */
s2k_status s2k_run_file_count(s2k_ctx *ctx, const char *path, const s2k_params *params, uint64_t batch_bases, s2k_counter *counter,
                              s2k_counts *totals, double *seconds);

#ifdef __cplusplus
}
#endif
#endif /* S2K_H */
