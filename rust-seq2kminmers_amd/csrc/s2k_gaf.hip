// s2k_gaf.hip -- the GAF lines of a batch's read walks, formatted on the device (include/s2k.h: s2k_walks_gaf).  The
// text is byte for byte what write_gaf_walks (writers.py) writes from the same arrays.
//
// A line is a head (name, read length, qstart, qend, +), the path (one token per step), a middle of fixed fields (path_len ..
// ns:i:), for an aligned walk NM:i: and cg:Z: with one token per run, and a newline.  Every part's length is known without writing
// it, so the call sizes first and writes second, and no lane walks a walk:
//  1. gaf_check_kernel, one lane per read and per walk: the rules of the header comment; one flag word.
//  2. gaf_steps_kernel, one lane per step: the token's length, 1 + digits(unitig >> 1); launch_scan_u32 gives P.
//  3. gaf_slots_kernel, one lane per run slot: whether the slot is LIVE -- inside [ops_off[w], ops_off[w] + n_ops[w]) of an unflagged
//     walk w, found by a search of ops_off; s2k_align_pairs leaves the slots behind a walk's runs untouched -- and, only then, its op
//     (legal or the flag is set), its token's length digits(len) + 1 and its run length; two scans give CP (bytes) and LP (bases).
//  4. gaf_lens_kernel, one lane per walk: the line's length from the lengths of its fields, two differences of P and CP, and the
//     name's length; where the path and the CIGAR start inside the line.  A scan gives line_off; a scan of n_steps gives the first
//     token of every walk, so that walks may share steps or stand in any order, as they may for the host writer.
//  5. the host reads the flag word, the bytes and the number of path tokens in ONE wait, and answers the sizes call, the refusals and
//     the capacity question: until here nothing outside the workspace was written.
//  6. gaf_fixed_kernel (a lane per walk: everything but the tokens), gaf_path_kernel (a lane per path token, its walk by a search of
//     the token offsets), gaf_cigar_kernel (a lane per live slot).  Consecutive lanes of the token kernels write neighbouring bytes.
// Every kernel before the wait guards its own reads (an offset that breaks a rule is not followed), so the check need not have
// passed for them to be safe; their results are then thrown away.  No atomic touches an output.
//
// Workspace (the context's grow-only count workspace): 12 B per step (token length, P), 24 B per run slot (token length, run
// length, CP, LP), 28 B per walk (length, the two starts, line_off, token offset), and the scans' block sums.
#include <algorithm>

#include "../../include/s2k.h"
#include "s2k_call.h"
#include "s2k_cigar_dev.h"
#include "s2k_dev.h"
#include "s2k_graph_dev.h"
#include "s2k_hostcopy.h"
#include "s2k_targets_dev.h"
#include "s2k_text_dev.h"

namespace s2k {
namespace {

enum : uint32_t { GF_BAD_RULE = 1u, GF_BAD_OP = 2u, GF_BAD_LINE = 4u };

struct GfIn {
    const uint64_t *walk_off, *first_step, *items, *path_len, *path_start, *path_end;
    const uint32_t *n_steps, *qstart, *qend;
    const uint32_t *unitig;
    const uint8_t *names; // with name_off, or both nullptr: the decimal first_read + r
    const uint64_t *name_off, *read_len;
    const uint32_t *edits, *aflags, *n_ops, *matches, *ops; // aflags nullptr: no alignments
    const uint64_t *ops_off;
    uint64_t n_reads, n_walks, n_all_steps, n_name_bytes, first_read, n_runs;
};

struct GfWs {
    uint32_t *steplen; // per step
    uint64_t *P;       // n_all_steps + 1
    uint32_t *tok, *rl; // per run slot: bytes of its token (0: not live), its run length
    uint64_t *CP, *LP;  // n_runs + 1
    uint32_t *len, *path_at, *cigar_at; // per walk: bytes of its line; where the path and the CIGAR start in it
    uint64_t *line_off, *tok_off;       // n_walks + 1
};

__device__ __forceinline__ bool steps_inside(const GfIn &in, uint64_t w) {
    const uint64_t a = in.first_step[w];
    return a <= in.n_all_steps && in.n_steps[w] <= in.n_all_steps - a;
}
__device__ __forceinline__ bool runs_inside(const GfIn &in, uint64_t w) {
    const uint64_t o = in.ops_off[w];
    return o <= in.n_runs && in.n_ops[w] <= in.n_runs - o;
}
__device__ __forceinline__ bool aligned(const GfIn &in, uint64_t w) { return in.aflags && in.aflags[w] == 0; }

__global__ __launch_bounds__(UT) void gaf_check_kernel(GfIn in, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x;
    bool ok = true;
    if (i <= in.n_reads) {
        const uint64_t a = in.walk_off[i];
        if ((i == 0 && a != 0) || (i == in.n_reads ? a != in.n_walks : a > in.walk_off[i + 1])) ok = false;
        if (in.name_off) {
            const uint64_t b = in.name_off[i];
            if ((i == 0 && b != 0) || (i == in.n_reads ? b > in.n_name_bytes : b > in.name_off[i + 1])) ok = false;
        }
    }
    if (i < in.n_walks) {
        if (!steps_inside(in, i) || in.qstart[i] > in.qend[i] || in.path_start[i] > in.path_end[i]) ok = false;
        if (in.aflags) {
            const uint64_t o = in.ops_off[i], e = in.ops_off[i + 1];
            if (o > e || !runs_inside(in, i) || (in.aflags[i] == 0 && in.n_ops[i] > e - o)) ok = false;
        }
    }
    if (i == in.n_walks && in.aflags && in.ops_off[i] > in.n_runs) ok = false;
    if (!ok) atomicOr(bad, GF_BAD_RULE);
}

__global__ __launch_bounds__(UT) void gaf_steps_kernel(GfIn in, GfWs ws) {
    const uint64_t s = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (s < in.n_all_steps) ws.steplen[s] = 1u + dec_digits(in.unitig[s] >> 1);
}

// the walk whose slots hold run slot i, when the slot is live; false otherwise
__device__ __forceinline__ bool live_slot(const GfIn &in, uint64_t i, uint64_t *w) {
    if (i < in.ops_off[0] || i >= in.ops_off[in.n_walks]) return false;
    *w = last_le(in.ops_off, 0, in.n_walks - 1, i);
    return in.aflags[*w] == 0 && i - in.ops_off[*w] < in.n_ops[*w];
}

__global__ __launch_bounds__(UT) void gaf_slots_kernel(GfIn in, GfWs ws, uint32_t *__restrict__ bad) {
    const uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= in.n_runs) return;
    uint32_t tok = 0, rl = 0;
    uint64_t w;
    if (live_slot(in, i, &w)) {
        const uint32_t v = in.ops[i], op = run_op(v);
        if (op != S2K_CIGAR_I && op != S2K_CIGAR_D && op != S2K_CIGAR_EQ && op != S2K_CIGAR_X) atomicOr(bad, GF_BAD_OP);
        rl = run_len(v);
        tok = dec_digits(rl) + 1u;
    }
    ws.tok[i] = tok;
    ws.rl[i] = rl;
}

// Walk w's line: its values, the digits of each, and where its parts lie.  line_parts() is what the length pass and the writer share.
struct Line {
    uint64_t r, name_a, name_n, rlen, plen, ps, pe, items, matches, block, path_n, cigar_n;
    uint32_t qs, qe, ns, edits;
    bool al;
    uint32_t d_rlen, d_qs, d_qe, d_plen, d_ps, d_pe, d_matches, d_block, d_items, d_ns, d_edits;
    uint64_t path_at, mid_at, cigar_at, total;
};
constexpr uint32_t MID_FIXED = 5 + 4 + 6 + 6; // five tabs, "\t255", "\tkm:i:", "\tns:i:"
constexpr uint32_t TAGS_FIXED = 6 + 6;        // "\tNM:i:", "\tcg:Z:"

__device__ __forceinline__ Line line_parts(const GfIn &in, const GfWs &ws, uint64_t w) {
    Line l;
    l.r = last_le(in.walk_off, 0, in.n_reads - 1, w);
    if (in.name_off) {
        const uint64_t a = in.name_off[l.r], b = in.name_off[l.r + 1];
        l.name_a = a, l.name_n = b >= a ? b - a : 0;
    } else {
        l.name_a = 0, l.name_n = dec_digits(in.first_read + l.r);
    }
    l.rlen = in.read_len ? in.read_len[l.r] : 0, l.d_rlen = in.read_len ? dec_digits(l.rlen) : 1u;
    l.qs = in.qstart[w], l.qe = in.qend[w], l.ns = in.n_steps[w];
    l.plen = in.path_len[w], l.ps = in.path_start[w], l.pe = in.path_end[w], l.items = in.items[w];
    const uint64_t a = in.first_step[w];
    l.path_n = ws.P[a + l.ns] - ws.P[a];
    l.al = aligned(in, w);
    l.matches = l.items, l.block = std::max<uint64_t>(l.qe - l.qs, l.pe - l.ps), l.edits = 0, l.cigar_n = 0;
    if (l.al) {
        const uint64_t o = in.ops_off[w], e = o + in.n_ops[w];
        l.matches = in.matches[w], l.block = ws.LP[e] - ws.LP[o], l.edits = in.edits[w], l.cigar_n = ws.CP[e] - ws.CP[o];
    }
    l.d_qs = dec_digits(l.qs), l.d_qe = dec_digits(l.qe), l.d_plen = dec_digits(l.plen), l.d_ps = dec_digits(l.ps), l.d_pe = dec_digits(l.pe);
    l.d_matches = dec_digits(l.matches), l.d_block = dec_digits(l.block), l.d_items = dec_digits(l.items), l.d_ns = dec_digits(l.ns);
    l.d_edits = dec_digits(l.edits);
    l.path_at = l.name_n + 1 + l.d_rlen + 1 + l.d_qs + 1 + l.d_qe + 3; // "\t+\t"
    l.mid_at = l.path_at + l.path_n;
    const uint64_t mid_n = MID_FIXED + l.d_plen + l.d_ps + l.d_pe + l.d_matches + l.d_block + l.d_items + l.d_ns;
    l.cigar_at = l.mid_at + mid_n + (l.al ? TAGS_FIXED + l.d_edits : 0u);
    l.total = l.cigar_at + l.cigar_n + 1;
    return l;
}

__global__ __launch_bounds__(UT) void gaf_lens_kernel(GfIn in, GfWs ws, uint32_t *__restrict__ bad) {
    const uint64_t w = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (w >= in.n_walks) return;
    uint32_t len = 0, path_at = 0, cigar_at = 0;
    if (steps_inside(in, w) && (!in.aflags || runs_inside(in, w))) { // (otherwise the check pass has set the flag)
        const Line l = line_parts(in, ws, w);
        if (l.total >> 32) atomicOr(bad, GF_BAD_LINE);
        len = (uint32_t)l.total, path_at = (uint32_t)l.path_at, cigar_at = (uint32_t)l.cigar_at;
    }
    ws.len[w] = len;
    ws.path_at[w] = path_at;
    ws.cigar_at[w] = cigar_at;
}

__device__ __forceinline__ uint8_t *put_field(uint8_t *p, uint64_t v, uint32_t nd) { // "\t<v>"
    *p = '\t';
    put_dec(p + 1, v, nd);
    return p + 1 + nd;
}

__global__ __launch_bounds__(UT) void gaf_fixed_kernel(GfIn in, GfWs ws, uint8_t *__restrict__ text) {
    const uint64_t w = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (w >= in.n_walks) return;
    const Line l = line_parts(in, ws, w);
    uint8_t *const line = text + ws.line_off[w];
    uint8_t *p = line;
    if (in.name_off) {
        for (uint64_t i = 0; i < l.name_n; i++) p[i] = in.names[l.name_a + i];
    } else {
        put_dec(p, in.first_read + l.r, (uint32_t)l.name_n);
    }
    p += l.name_n;
    if (in.read_len) {
        p = put_field(p, l.rlen, l.d_rlen);
    } else {
        p[0] = '\t', p[1] = '*', p += 2;
    }
    p = put_field(p, l.qs, l.d_qs);
    p = put_field(p, l.qe, l.d_qe);
    put_text(p, "\t+\t", 3);
    p = line + l.mid_at;
    p = put_field(p, l.plen, l.d_plen);
    p = put_field(p, l.ps, l.d_ps);
    p = put_field(p, l.pe, l.d_pe);
    p = put_field(p, l.matches, l.d_matches);
    p = put_field(p, l.block, l.d_block);
    put_text(p, "\t255\tkm:i:", 10);
    put_dec(p + 10, l.items, l.d_items);
    p += 10 + l.d_items;
    put_text(p, "\tns:i:", 6);
    put_dec(p + 6, l.ns, l.d_ns);
    p += 6 + l.d_ns;
    if (l.al) {
        put_text(p, "\tNM:i:", 6);
        put_dec(p + 6, l.edits, l.d_edits);
        p += 6 + l.d_edits;
        put_text(p, "\tcg:Z:", 6);
    }
    line[l.total - 1] = '\n';
}

__global__ __launch_bounds__(UT) void gaf_path_kernel(GfIn in, GfWs ws, uint64_t n_tokens, uint8_t *__restrict__ text) {
    const uint64_t j = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (j >= n_tokens) return;
    const uint64_t w = last_le(ws.tok_off, 0, in.n_walks - 1, j), a = in.first_step[w], s = a + (j - ws.tok_off[w]);
    const uint32_t U = in.unitig[s];
    uint8_t *p = text + ws.line_off[w] + ws.path_at[w] + (ws.P[s] - ws.P[a]);
    *p = (U & 1u) ? '<' : '>';
    put_dec(p + 1, U >> 1, ws.steplen[s] - 1u);
}

__global__ __launch_bounds__(UT) void gaf_cigar_kernel(GfIn in, GfWs ws, uint8_t *__restrict__ text) {
    const uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x;
    if (i >= in.n_runs) return;
    const uint32_t tok = ws.tok[i];
    if (tok == 0) return;
    const uint64_t w = last_le(in.ops_off, 0, in.n_walks - 1, i);
    const uint32_t v = in.ops[i], op = run_op(v);
    uint8_t *p = text + ws.line_off[w] + ws.cigar_at[w] + (ws.CP[i] - ws.CP[in.ops_off[w]]);
    put_dec(p, run_len(v), tok - 1u);
    p[tok - 1u] = op == S2K_CIGAR_I ? 'I' : op == S2K_CIGAR_D ? 'D' : op == S2K_CIGAR_EQ ? '=' : 'X';
}

inline unsigned blocks_for(uint64_t n) { return (unsigned)((n + UT - 1) / UT); }
constexpr uint64_t GF_MAX_LANES = 1ull << 39; // one lane per item in blocks of UT: the grid's x stays below 2^31

} // namespace
} // namespace s2k

using namespace s2k;

extern "C" {

s2k_status s2k_walks_gaf(s2k_ctx *ctx, uint64_t n_reads, const s2k_walk_out *walks, uint64_t n_walks, const uint32_t *d_step_unitig, uint64_t n_steps,
                         const uint8_t *d_names, const uint64_t *d_name_off, uint64_t n_name_bytes, uint64_t first_read, const uint64_t *d_read_len,
                         const s2k_align_out *al, uint8_t *d_text, uint64_t capacity, uint64_t *d_line_off, uint64_t *n_bytes) {
    if (n_bytes) *n_bytes = 0;
    if (!ctx || !n_bytes || !walks || !walks->walk_off || (d_names == nullptr) != (d_name_off == nullptr)) return S2K_ERR_INVALID_ARG;
    if (n_walks && (!walks->first_step || !walks->n_steps || !walks->items || !walks->qstart || !walks->qend || !walks->path_len || !walks->path_start ||
                    !walks->path_end))
        return S2K_ERR_INVALID_ARG;
    if (n_steps && !d_step_unitig) return S2K_ERR_INVALID_ARG;
    if (al && (!al->flags || !al->ops_off || (n_walks && (!al->edits || !al->n_ops || !al->matches)) || (al->capacity && !al->ops))) return S2K_ERR_INVALID_ARG;
    Call c(ctx, "s2k_walks_gaf");
    const uint64_t n_runs = al ? al->capacity : 0;
    if (n_walks >= (1ull << 31)) return c.invalid("2^31 walks or more");
    if (n_reads >= GF_MAX_LANES || n_steps >= GF_MAX_LANES || n_runs >= GF_MAX_LANES) return c.invalid("too many reads, steps or runs for one call");
    if (n_walks && n_reads == 0) return c.invalid("walks without reads");
    if (first_read + n_reads < first_read) return c.invalid("first_read + n_reads passes 2^64");
    if (hipSetDevice(ctx_device(ctx)) != hipSuccess) return S2K_ERR_DEVICE;
    if (n_walks == 0) { // no walks: no text, and no input is read
        if (d_line_off) {
            c.zero(d_line_off, 8);
            if (!c.sync()) return c.device_error();
        }
        return S2K_OK;
    }
    Layout L;
    const auto words_p = L.bytes<uint32_t>(16);
    const auto steplen_p = L.take<uint32_t>(n_steps);
    const auto P_p = L.take<uint64_t>(n_steps + 1);
    const auto tok_p = L.take<uint32_t>(n_runs), rl_p = L.take<uint32_t>(n_runs);
    const auto CP_p = L.take<uint64_t>(n_runs + 1), LP_p = L.take<uint64_t>(n_runs + 1);
    const auto len_p = L.take<uint32_t>(n_walks), path_at_p = L.take<uint32_t>(n_walks), cigar_at_p = L.take<uint32_t>(n_walks);
    const auto line_off_p = L.take<uint64_t>(n_walks + 1), tok_off_p = L.take<uint64_t>(n_walks + 1);
    const auto tmp_p = L.bytes<uint64_t>(scan_tmp_bytes(std::max(std::max(n_steps, n_runs), n_walks)));
    char *w = L.alloc(ctx);
    if (!w) return c.nomem();
    uint32_t *bad = words_p(w);
    const GfIn in{walks->walk_off, walks->first_step, walks->items, walks->path_len, walks->path_start, walks->path_end, walks->n_steps, walks->qstart,
                  walks->qend, d_step_unitig, d_names, d_name_off, d_read_len, al ? al->edits : nullptr, al ? al->flags : nullptr, al ? al->n_ops : nullptr,
                  al ? al->matches : nullptr, al ? al->ops : nullptr, al ? al->ops_off : nullptr, n_reads, n_walks, n_steps, n_name_bytes, first_read, n_runs};
    const GfWs ws{steplen_p(w), P_p(w), tok_p(w), rl_p(w), CP_p(w), LP_p(w), len_p(w), path_at_p(w), cigar_at_p(w), line_off_p(w), tok_off_p(w)};
    uint64_t total = 0, n_tokens = 0;
    const uint32_t hbad = c.check(
        bad, 16, bad,
        [&] {
            c.launch(gaf_check_kernel, blocks_for(std::max(n_reads, n_walks) + 1), UT, in, bad);
            if (n_steps) c.launch(gaf_steps_kernel, blocks_for(n_steps), UT, in, ws);
            c.scan(ws.steplen, n_steps, ws.P, tmp_p(w));
            if (n_runs) c.launch(gaf_slots_kernel, blocks_for(n_runs), UT, in, ws, bad);
            c.scan(ws.tok, n_runs, ws.CP, tmp_p(w));
            c.scan(ws.rl, n_runs, ws.LP, tmp_p(w));
            c.launch(gaf_lens_kernel, blocks_for(n_walks), UT, in, ws, bad);
            c.scan(ws.len, n_walks, ws.line_off, tmp_p(w));
            c.scan(walks->n_steps, n_walks, ws.tok_off, tmp_p(w));
        },
        [&] {
            c.fetch(&total, ws.line_off + n_walks, 8);
            c.fetch(&n_tokens, ws.tok_off + n_walks, 8);
        });
    if (!c.ok()) return c.device_error();
    if (hbad & GF_BAD_RULE)
        return c.invalid("walk_off that does not run from 0 to n_walks without decreasing, a walk whose steps pass n_steps, qstart above qend, path_start "
                         "above path_end, name_off that does not run from 0 without decreasing or passes n_name_bytes, ops_off that decreases or passes "
                         "the runs there are, or n_ops above a walk's slots");
    if (hbad & GF_BAD_OP) return c.invalid("a run with an unknown code in a walk that is aligned");
    if (hbad & GF_BAD_LINE) return c.invalid("a line of 2^32 bytes or more");
    if (n_tokens >= GF_MAX_LANES) return c.invalid("too many steps for one call");
    *n_bytes = total;
    if (d_text && total > capacity) return S2K_ERR_CAPACITY;
    if (d_line_off) c.copy(d_line_off, ws.line_off, (n_walks + 1) * 8, hipMemcpyDeviceToDevice);
    if (d_text) {
        c.launch(gaf_fixed_kernel, blocks_for(n_walks), UT, in, ws, d_text);
        if (n_tokens) c.launch(gaf_path_kernel, blocks_for(n_tokens), UT, in, ws, n_tokens, d_text);
        if (n_runs) c.launch(gaf_cigar_kernel, blocks_for(n_runs), UT, in, ws, d_text);
    }
    if (!c.sync()) return c.device_error();
    return S2K_OK;
}

} // extern "C"
