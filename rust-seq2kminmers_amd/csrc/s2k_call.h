// s2k_call.h -- the host scaffold of an entry point of the count, table and graph calls (plain C++, no device code): the 256-byte
// round-up, the layout of a call's pieces in the context's grow-only count workspace, and the running error state of a call that
// queues its work on the context's stream and waits with ctx_sync only (the queue budget that tests/test_queue_budget.py pins).  The minimizer /
// k-min-mer pipeline (s2k_api.hip) has its own conventions and does not use this.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/s2k.h"
#include "s2k_dev.h"
#include "s2k_hostcopy.h"

namespace s2k {
namespace {

inline size_t al(size_t b) { return (b + 255) & ~(size_t)255; }

// A call's workspace, in two passes: take() every piece in order (each starts on a 256-byte boundary), alloc() once, then give the
// base to a piece to get its typed address.  Offset and type travel together.
class Layout {
  public:
    template <typename T>
    struct Piece {
        size_t off;
        T *operator()(char *w) const { return (T *)(w + off); }
    };
    template <typename T>
    Piece<T> take(uint64_t n) { return bytes<T>(n * sizeof(T)); }
    template <typename T>
    Piece<T> bytes(size_t b) {
        const Piece<T> p{off_};
        off_ += al(b);
        return p;
    }
    char *alloc(s2k_ctx *ctx) const { return (char *)ctx_count_table(ctx, off_); } // nullptr: allocation failed

  private:
    size_t off_ = 0;
};

// One entry point's work on the context's stream.  Every operation is skipped once one has failed, so a call site queues step after
// step and asks once, at its host wait.  The three refusals set the context's error text "<name>: <what>" and return the status.
struct Call {
    s2k_ctx *ctx;
    const char *name; // the entry point, as the error texts name it
    hipStream_t st;
    hipError_t e = hipSuccess;

    Call(s2k_ctx *c, const char *entry) : ctx(c), name(entry), st(ctx_stream(c)) {}
    bool ok() const { return e == hipSuccess; }
    void zero(void *d, size_t bytes) { fill(d, 0, bytes); }
    void fill(void *d, int byte, size_t bytes) {
        if (ok()) e = hipMemsetAsync(d, byte, bytes, st);
    }
    void copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        if (ok()) e = hipMemcpyAsync(dst, src, bytes, kind, st);
    }
    void fetch(void *host, const void *dev, size_t bytes) { copy(host, dev, bytes, hipMemcpyDeviceToHost); }
    void launched() { // after hipLaunchKernelGGL
        if (ok()) e = hipGetLastError();
    }
    template <typename K, typename... A>
    void launch(K kernel, unsigned grid, unsigned block, const A &...args) { // the kernel on st, and its launch error
        if (!ok()) return;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, args...);
        e = hipGetLastError();
    }
    void scan(const uint32_t *in, uint64_t n, uint64_t *out /*n+1*/, uint64_t *tmp) {
        if (ok()) e = launch_scan_u32(in, n, out, tmp, 0, st);
    }
    bool sync() { // the host wait; false: the call has failed, here or earlier
        if (ok()) e = ctx_sync(ctx);
        return ok();
    }
    // zero `bytes` at z, queue() the kernels that set *flag (inside z's range), fetch it, more() (the caller's further fetches), wait:
    // the flag, for the caller's refusal
    template <typename F, typename M>
    uint32_t check(void *z, size_t bytes, const uint32_t *flag, F queue, M more) {
        uint32_t h = 0;
        zero(z, bytes);
        if (ok()) {
            queue();
            launched();
        }
        fetch(&h, flag, 4);
        more();
        sync();
        return h;
    }
    template <typename F>
    uint32_t check(void *z, size_t bytes, const uint32_t *flag, F queue) {
        return check(z, bytes, flag, queue, [] {});
    }

    s2k_status refuse(s2k_status s, const char *what) const {
        ctx_set_error(ctx, (std::string(name) + ": " + what).c_str());
        return s;
    }
    s2k_status device_error(const char *what = "HIP error") const { return refuse(S2K_ERR_DEVICE, what); }
    s2k_status invalid(const char *what) const { return refuse(S2K_ERR_INVALID_ARG, what); }
    s2k_status nomem(const char *what = "workspace allocation") const { return refuse(S2K_ERR_NOMEM, what); }
};

// km_off[0], km_off[n_reads], mn_off[0], mn_off[n_reads] (mn_off may be NULL: zeros), and the host wait
struct Ends {
    uint64_t km0, n_items, mn0, n_triples;
};
inline Ends read_ends(Call &c, const uint64_t *km_off, const uint64_t *mn_off, uint64_t n_reads) {
    Ends e{0, 0, 0, 0};
    c.fetch(&e.km0, km_off, 8);
    c.fetch(&e.n_items, km_off + n_reads, 8);
    if (mn_off) {
        c.fetch(&e.mn0, mn_off, 8);
        c.fetch(&e.n_triples, mn_off + n_reads, 8);
    }
    c.sync();
    return e;
}

} // namespace
} // namespace s2k
