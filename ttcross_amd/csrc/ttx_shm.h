// ttx_shm.h -- the built-in node-local host transport over POSIX shared memory (host only: no HIP and no engine in here).
//
// For jobs whose processes share a node but cannot use RCCL (several ranks on ONE GPU -- RCCL refuses that -- or no
// librccl), and for launchers without MPI (the Fortran drop-in layer): the ttx_transport primitives implemented on a
// shared segment.  Point-to-point: one mailbox per (receiver, side) with a sequence / acknowledge pair; all-reduce: every
// rank deposits its vector, a sense-reversing barrier, every rank folds the W vectors in rank order (so all ranks get
// the identical bits), a second barrier before the slots are reused.  Waits are bounded (ShmTransport::bound) and report failure.
// Attaching is a handshake on a per-initialisation NONCE, so that a rank can never end up on a segment that rank 0 did not
// create in THIS call (a segment left by a crashed job, or the one of the previous dtt_dmrgg of the same job, still carries
// ready = 1 and old counters): rank 0 unlinks the name, creates a fresh segment and publishes a random nonce; rank r copies the
// nonce it sees into hello[r] and waits for go == that nonce, which rank 0 sets once every hello matches.  A segment whose go
// is already set before the rank said hello is stale by construction; while it waits, a rank re-checks that the NAME still
// leads to the inode it has mapped (rank 0's unlink + create changes it) and starts over if not.
// ttx_comm_init_shm of ttx_engine.hip sizes the segment and wires the transport into an engine; tests/shm_main.cpp runs it
// between forked processes on the CPU.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <functional>
#include <random>
#include <string>
#include <thread>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include "../../include/ttx.h"

struct ShmHeader {
    std::atomic<uint32_t> ready, arrived, sense;
    uint32_t W; uint64_t msz, redcap;
    std::atomic<uint64_t> nonce, go;
    std::atomic<uint64_t> hello[256];
};
static_assert(sizeof(ShmHeader) <= 4096, "the header shares the first page of the segment");
struct ShmBox { std::atomic<uint64_t> seq, ack; uint64_t bytes; };
struct ShmTransport {
    void *base = nullptr; size_t size = 0; std::string name; int rank = 0, W = 1; bool owner = false;
    ShmHeader *hd = nullptr;
    size_t msz = 0, redcap = 0;
    uint32_t my_sense = 0;
    double bound = 60.0;                // seconds a wait or an attach may take; the engine never sets it
    ShmBox *box(int r, int side) const { return (ShmBox *)((char *)base + 4096 + ((size_t)r * 2 + side) * (64 + msz)); }   // side 0: from the left, 1: from the right
    char *boxdata(int r, int side) const { return (char *)box(r, side) + 64; }
    double *red(int r) const { return (double *)((char *)base + 4096 + (size_t)W * 2 * (64 + msz) + (size_t)r * redcap * sizeof(double)); }
};
inline bool shm_wait(const ShmTransport *T, const std::function<bool()> &cond)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; spins++) {
        if (cond()) return true;
        if ((spins & 1023u) == 1023u) {
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > T->bound) return false;
            std::this_thread::yield();
        }
    }
}
inline int shm_barrier(ShmTransport *T)
{
    T->my_sense ^= 1u;
    if (T->hd->arrived.fetch_add(1u, std::memory_order_acq_rel) + 1u == (uint32_t)T->W) {
        T->hd->arrived.store(0u, std::memory_order_relaxed);
        T->hd->sense.store(T->my_sense, std::memory_order_release);
        return 0;
    }
    return shm_wait(T, [&] { return T->hd->sense.load(std::memory_order_acquire) == T->my_sense; }) ? 0 : 1;
}
// the two primitives of a ttx_transport (include/ttx.h); ctx is the ShmTransport
inline int shm_sendrecv(void *ctx, int to, const void *sbuf, int64_t ns, int from, void *rbuf, int64_t nr)
{
    ShmTransport *T = (ShmTransport *)ctx;
    if ((size_t)ns > T->msz || (size_t)nr > T->msz) return 1;
    if (to >= 0) {                                   // I am the left neighbour of `to` when to == rank + 1: its side-0 box
        const int side = (to == T->rank + 1) ? 0 : 1;
        ShmBox *b = T->box(to, side);
        if (!shm_wait(T, [&] { return b->ack.load(std::memory_order_acquire) == b->seq.load(std::memory_order_relaxed); })) return 1;
        memcpy(T->boxdata(to, side), sbuf, (size_t)ns);
        b->bytes = (uint64_t)ns;
        b->seq.fetch_add(1u, std::memory_order_release);
    }
    if (from >= 0) {
        const int side = (from == T->rank - 1) ? 0 : 1;
        ShmBox *b = T->box(T->rank, side);
        if (!shm_wait(T, [&] { return b->seq.load(std::memory_order_acquire) != b->ack.load(std::memory_order_relaxed); })) return 1;
        memcpy(rbuf, T->boxdata(T->rank, side), (size_t)std::min<uint64_t>((uint64_t)nr, b->bytes));
        b->ack.fetch_add(1u, std::memory_order_release);
    }
    return 0;
}
inline int shm_allreduce(void *ctx, double *buf, int64_t count, int op)
{
    ShmTransport *T = (ShmTransport *)ctx;
    if ((size_t)count > T->redcap) return 1;
    memcpy(T->red(T->rank), buf, sizeof(double) * (size_t)count);
    if (shm_barrier(T)) return 1;
    for (int64_t i = 0; i < count; i++) {
        double a = T->red(0)[i];
        for (int r = 1; r < T->W; r++) a = op ? std::max(a, T->red(r)[i]) : a + T->red(r)[i];
        buf[i] = a;
    }
    return shm_barrier(T);
}
// unmap the segment, and take the name away where this rank created it; the transport is unattached afterwards
inline void shm_close(ShmTransport *T)
{
    if (T->base) munmap(T->base, T->size);
    if (T->owner) shm_unlink(T->name.c_str());
    T->base = nullptr; T->hd = nullptr; T->owner = false;
}
// Attach rank `rank` of W to the segment `name` (as the caller gave it: the messages use it, the segment's name gets the '/' it may
// lack) with mailboxes of msz bytes and all-reduce slots of redcap doubles.  TTX_OK: *T is attached, every rank has said hello to
// this rank 0's nonce.  Otherwise the code, the message in *errtext, and *T unattached.  T->bound holds as the caller left it.
inline int shm_attach(const char *name, int rank, int W, size_t msz, size_t redcap, ShmTransport *T, std::string *errtext)
{
    auto refuse = [&](int code, const std::string &text) { shm_close(T); *errtext = "ttx_comm_init_shm: " + text; return code; };
    T->name = std::string(name[0] == '/' ? "" : "/") + name;
    T->rank = rank; T->W = W; T->msz = msz; T->redcap = redcap;
    T->size = 4096 + (size_t)W * 2 * (64 + msz) + (size_t)W * redcap * sizeof(double);
    const auto t_start = std::chrono::steady_clock::now();
    auto elapsed = [&] { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count(); };
    if (rank == 0) {
        shm_unlink(T->name.c_str());
        int fd = shm_open(T->name.c_str(), O_CREAT | O_EXCL | O_RDWR, 0600);
        if (fd < 0 || ftruncate(fd, (off_t)T->size) != 0) { if (fd >= 0) close(fd); return refuse(TTX_EHIP, std::string("cannot create ") + name); }
        T->owner = true;
        T->base = mmap(nullptr, T->size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        if (T->base == MAP_FAILED) { T->base = nullptr; return refuse(TTX_EHIP, "mmap failed"); }
        T->hd = (ShmHeader *)T->base;          // a fresh segment is zero-filled: sequence numbers, counters, sense, go and hello start at 0
        T->hd->W = (uint32_t)W; T->hd->msz = msz; T->hd->redcap = redcap;
        std::random_device rd;
        uint64_t nonce = ((uint64_t)rd() << 32) ^ (uint64_t)rd() ^ ((uint64_t)getpid() << 17) ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
        if (nonce == 0) nonce = 1;
        T->hd->nonce.store(nonce, std::memory_order_relaxed);
        T->hd->ready.store(1u, std::memory_order_release);
        const bool all = shm_wait(T, [&] {
            for (int r = 1; r < W; r++) if (T->hd->hello[r].load(std::memory_order_acquire) != nonce) return false;
            return true;
        });
        if (!all) return refuse(TTX_EHIP, "not all " + std::to_string(W) + " ranks attached to " + name);
        T->hd->go.store(nonce, std::memory_order_release);
        return TTX_OK;
    }
    bool joined = false, mismatch = false;
    while (!joined && elapsed() < T->bound) {
        int fd = shm_open(T->name.c_str(), O_RDWR, 0600);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0 || (size_t)st.st_size < T->size) { if (fd >= 0) close(fd); std::this_thread::sleep_for(std::chrono::milliseconds(2)); continue; }
        const ino_t ino = st.st_ino;
        void *base = mmap(nullptr, T->size, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
        close(fd);
        if (base == MAP_FAILED) return refuse(TTX_EHIP, "mmap failed");
        ShmHeader *hd = (ShmHeader *)base;
        auto still_current = [&] {          // does the name still lead to the segment that is mapped here?
            int f2 = shm_open(T->name.c_str(), O_RDWR, 0600);
            struct stat s2;
            const bool same = f2 >= 0 && fstat(f2, &s2) == 0 && s2.st_ino == ino;
            if (f2 >= 0) close(f2);
            return same;
        };
        bool restart = false, said = false;
        uint64_t nonce = 0;
        auto t_chk = std::chrono::steady_clock::now();
        while (!restart && elapsed() < T->bound) {
            if (!said && hd->ready.load(std::memory_order_acquire) == 1u) {
                mismatch = hd->W != (uint32_t)W || hd->msz != msz || hd->redcap != redcap;
                nonce = hd->nonce.load(std::memory_order_relaxed);
                if (mismatch || hd->go.load(std::memory_order_acquire) == nonce) {
                    // another problem's segment, or one whose initialisation is over: not ours -- wait for rank 0 to replace the name
                    while (elapsed() < T->bound && still_current()) std::this_thread::sleep_for(std::chrono::milliseconds(2));
                    restart = true;
                    break;
                }
                hd->hello[rank].store(nonce, std::memory_order_release);
                said = true;
            }
            if (said && hd->go.load(std::memory_order_acquire) == nonce) { joined = true; break; }
            if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_chk).count() > 0.02) {
                t_chk = std::chrono::steady_clock::now();
                if (!still_current()) restart = true;
            }
            std::this_thread::yield();
        }
        if (joined) { T->base = base; T->hd = hd; }
        else munmap(base, T->size);
    }
    if (joined) return TTX_OK;
    return mismatch ? refuse(TTX_EINVAL, std::string("the ranks disagree about the problem (or ") + name + " belongs to another job)")
                    : refuse(TTX_EHIP, std::string("rank 0 did not create ") + name + " (or never saw every rank)");
}
