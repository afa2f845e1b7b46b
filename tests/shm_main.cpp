// Stand-alone check of ttcross_amd/csrc/ttx_shm.h (host code only): the node-local transport between forked processes, one
// process per rank, on segments named after this program's pid.  The ring exchange of hostfn_xfer, the rank-order all-reduce, a
// segment left behind by a job that never closed it, the three ways an attach fails (with the bound at 0.3 s) and the close.
// One line per case (tests/test_shm_cpu.py holds them); built plain and with -fsanitize=address,undefined by that test.
#include "ttx_shm.h"

#include <cstdio>
#include <vector>
#include <sys/wait.h>

static std::vector<std::string> g_names;      // every name handed out: whatever a failed case left behind is unlinked at the end
static std::string seg(const char *tag)
{
    static const long pid = (long)getpid();
    g_names.push_back("ttx_shm_test_" + std::to_string(pid) + "_" + tag);
    return g_names.back();
}
static bool name_exists(const std::string &name)
{
    const int fd = shm_open(("/" + name).c_str(), O_RDWR, 0600);
    if (fd >= 0) close(fd);
    return fd >= 0;
}
static const char *code_name(int rc) { return rc == TTX_OK ? "TTX_OK" : rc == TTX_EHIP ? "TTX_EHIP" : rc == TTX_EINVAL ? "TTX_EINVAL" : "another code"; }
// the message with the segment's name taken out: the name carries a pid
static std::string anonymous(std::string text, const std::string &name)
{
    for (size_t at; (at = text.find(name)) != std::string::npos;) text.replace(at, name.size(), "NAME");
    return text;
}

// a job of W ranks: rank r runs fn(r) in a child of its own, delay_ms[r] after the start; the OR of what the ranks returned
// (0: all was well; 128: a rank died)
template <class FN>
static int job(int W, FN fn, const int *delay_ms = nullptr)
{
    pid_t pid[8];
    fflush(nullptr);
    for (int r = 0; r < W; r++) {
        pid[r] = fork();
        if (pid[r] == 0) {
            if (delay_ms && delay_ms[r]) std::this_thread::sleep_for(std::chrono::milliseconds(delay_ms[r]));
            _exit(fn(r) & 127);
        }
    }
    int all = 0;
    for (int r = 0; r < W; r++) {
        int st = 0;
        if (pid[r] < 0 || waitpid(pid[r], &st, 0) != pid[r] || !WIFEXITED(st)) all |= 128;
        else all |= WEXITSTATUS(st);
    }
    return all;
}
#define NEED(bit, c) do { if (!(c)) { fprintf(stderr, "rank %d, line %d: %s\n", rank, __LINE__, #c); return bit; } } while (0)

// what the engine does with a transport: attach, then the barrier after which rank 0 may unlink the name (a rank whose peer
// failed a check gives up after 15 s here)
static int attach(ShmTransport *T, const std::string &name, int rank, int W, size_t msz = 64, size_t redcap = 8)
{
    std::string text;
    T->bound = 15.0;
    const int rc = shm_attach(name.c_str(), rank, W, msz, redcap, T, &text);
    if (rc) { fprintf(stderr, "rank %d: %s\n", rank, text.c_str()); return rc; }
    return shm_barrier(T) ? -1 : 0;
}

static unsigned char payload(int sender, int round, int dir, int j) { return (unsigned char)(1 + 97 * sender + 31 * round + 13 * dir + j); }
// five rounds of the two calls of hostfn_xfer: (to = right, from = left), then (to = left, from = right), -1 at the ends
static int ring(const std::string &name, int rank, int W)
{
    ShmTransport T;
    NEED(1, attach(&T, name, rank, W) == 0);
    const int left = rank > 0 ? rank - 1 : -1, right = rank + 1 < W ? rank + 1 : -1;
    static const int NS[5] = {0, 1, 64, 17, 64}, NR[5] = {0, 1, 64, 64, 64};      // round 3: ns < nr
    for (int k = 0; k < 5; k++)
        for (int dir = 0; dir < 2; dir++) {
            const int to = dir ? left : right, from = dir ? right : left;
            unsigned char s[64], r[64];
            for (int j = 0; j < 64; j++) s[j] = payload(rank, k, dir, j);
            memset(r, 0xEE, sizeof r);
            NEED(1, shm_sendrecv(&T, to, s, NS[k], from, r, NR[k]) == 0);
            for (int j = 0; j < 64; j++) NEED(1, r[j] == (from >= 0 && j < NS[k] ? payload(from, k, dir, j) : 0xEE));   // beyond ns: untouched
        }
    NEED(1, shm_barrier(&T) == 0);
    shm_close(&T);
    return 0;
}

static int overlong(const std::string &name, int rank)
{
    ShmTransport T;
    NEED(1, attach(&T, name, rank, 2) == 0);
    unsigned char s[65], r[64];
    memset(s, 0x55, sizeof s);
    if (rank == 0) NEED(1, shm_sendrecv(&T, 1, s, 65, -1, nullptr, 0) == 1);
    NEED(1, shm_barrier(&T) == 0);
    if (rank == 1) {                            // my box from the left is as the fresh segment had it
        NEED(1, T.box(1, 0)->seq.load() == 0 && T.box(1, 0)->bytes == 0);
        for (int j = 0; j < 64; j++) NEED(1, T.boxdata(1, 0)[j] == 0);
    }
    NEED(1, shm_barrier(&T) == 0);
    NEED(1, shm_sendrecv(&T, rank == 0 ? 1 : -1, s, 64, rank == 1 ? 0 : -1, r, 64) == 0);     // and it still works
    if (rank == 1) NEED(1, memcmp(r, s, 64) == 0);
    NEED(1, shm_barrier(&T) == 0);
    shm_close(&T);
    return 0;
}

// bit 0: the sum of one, bit 1: the sum of redcap, bit 2: the maximum, bit 3: redcap + 1
static int reduce(const std::string &name, int rank)
{
    const size_t redcap = 8;
    ShmTransport T;
    NEED(15, attach(&T, name, rank, 3, 64, redcap) == 0);
    static const double mine[3] = {1e16, 1.0, -1e16};   // in rank order (1e16 + 1.0) + -1e16 = 0.0; any other order gives 1.0
    double b[redcap + 1] = {mine[rank]};
    NEED(1, shm_allreduce(&T, b, 1, 0) == 0 && b[0] == 0.0);
    for (size_t i = 0; i < redcap; i++) b[i] = mine[rank];
    NEED(2, shm_allreduce(&T, b, redcap, 0) == 0);
    for (size_t i = 0; i < redcap; i++) NEED(2, b[i] == 0.0);
    for (size_t i = 0; i < redcap; i++) b[i] = (int)(i % 3) == rank ? 100.0 + i : -1.0 - i - rank;
    NEED(4, shm_allreduce(&T, b, redcap, 1) == 0);
    for (size_t i = 0; i < redcap; i++) NEED(4, b[i] == 100.0 + i);
    for (size_t i = 0; i <= redcap; i++) b[i] = rank + 0.5;
    NEED(8, shm_allreduce(&T, b, redcap + 1, 0) == 1);
    for (size_t i = 0; i <= redcap; i++) NEED(8, b[i] == rank + 0.5);
    NEED(15, shm_barrier(&T) == 0);
    shm_close(&T);
    return 0;
}

// a failed attach of one rank with the bound at `bound` seconds: the code and the message, as a line
static std::string refused(const std::string &name, int rank, size_t msz, double bound)
{
    ShmTransport T;
    T.bound = bound;
    std::string text;
    const int rc = shm_attach(name.c_str(), rank, 2, msz, 8, &T, &text);
    return std::string(code_name(rc)) + " \"" + anonymous(text, name) + "\"" + (T.base || T.owner ? " and the transport is still attached" : "");
}

int main()
{
    int bad = 0;
    auto line = [&](bool ok, const char *what) { printf("%s: %s\n", what, ok ? "ok" : "FAILED"); bad += !ok; };
    for (int W : {3, 2}) {
        const std::string name = seg(W == 3 ? "ring3" : "ring2");
        const int rc = job(W, [&](int rank) { return ring(name, rank, W); });
        line(rc == 0, W == 3 ? "ring of 3 ranks, 5 rounds, messages of 0, 1, 64 and 17 of 64 bytes" : "ring of 2 ranks, 5 rounds, messages of 0, 1, 64 and 17 of 64 bytes");
        if (W == 3) line(!name_exists(name), "close: the name is gone after the owner closed");
    }
    {
        const std::string name = "/" + seg("long");     // a name that brings its '/'
        line(job(2, [&](int rank) { return overlong(name, rank); }) == 0, "message of msz + 1 bytes: refused, nothing written");
    }
    {
        const std::string name = seg("reduce");
        const int rc = job(3, [&](int rank) { return reduce(name, rank); });
        line(!(rc & (128 | 1)), "all-reduce of 3 ranks, sum, count 1: 1e16 + 1.0 + -1e16 is 0.0 on every rank");
        line(!(rc & (128 | 2)), "all-reduce of 3 ranks, sum, count redcap: 0.0 everywhere");
        line(!(rc & (128 | 4)), "all-reduce of 3 ranks, max: the maximum on every rank");
        line(!(rc & (128 | 8)), "all-reduce of redcap + 1: refused, the vector untouched");
    }
    {
        // a first job attaches and leaves without closing: go is set and the name stays; a second job under the same name, its
        // rank 1 50 ms ahead of its rank 0, must not end up on that segment
        const std::string name = seg("stale");
        const int first = job(2, [&](int rank) { ShmTransport T; NEED(1, attach(&T, name, rank, 2) == 0); return 0; });
        line(first == 0 && name_exists(name), "stale segment: a job of 2 ranks left without closing, the name is still there");
        const int delay[2] = {50, 0};
        const int second = job(2, [&](int rank) {
            ShmTransport T;
            NEED(1, attach(&T, name, rank, 2) == 0);
            unsigned char s[8], r[8] = {0};
            for (int j = 0; j < 8; j++) s[j] = payload(rank, 0, 0, j);
            NEED(1, shm_sendrecv(&T, 1 - rank, s, 8, 1 - rank, r, 8) == 0);
            for (int j = 0; j < 8; j++) NEED(1, r[j] == payload(1 - rank, 0, 0, j));
            NEED(1, shm_barrier(&T) == 0);
            shm_close(&T);
            return 0;
        }, delay);
        line(second == 0 && !name_exists(name), "stale segment: the next job under that name attached, exchanged a message and closed");
    }
    {
        const std::string name = seg("alone0");
        printf("rank 0 alone: %s\n", refused(name, 0, 64, 0.3).c_str());
        line(!name_exists(name), "rank 0 alone: the name is gone");
    }
    printf("rank 1 alone: %s\n", refused(seg("alone1"), 1, 64, 0.3).c_str());
    {
        // rank 0 (in a child, with mailboxes of 128 bytes) keeps its segment for a second; rank 1 comes with 64
        const std::string name = seg("msz");
        fflush(nullptr);
        const pid_t child = fork();
        if (child == 0) { const bool as_expected = refused(name, 0, 128, 1.0) == "TTX_EHIP \"ttx_comm_init_shm: not all 2 ranks attached to NAME\""; _exit(as_expected ? 0 : 1); }
        for (int ms = 0; ms < 5000 && !name_exists(name); ms++) std::this_thread::sleep_for(std::chrono::milliseconds(1));     // rank 1's 0.3 s start once the name is there
        printf("rank 1 with another msz: %s\n", refused(name, 1, 64, 0.3).c_str());
        int st = -1;
        line(child > 0 && waitpid(child, &st, 0) == child && WIFEXITED(st) && WEXITSTATUS(st) == 0 && !name_exists(name), "rank 1 with another msz: rank 0 gave up and took the name away");
    }
    for (const auto &name : g_names) shm_unlink(("/" + name).c_str());
    printf(bad ? "shm: %d checks FAILED\n" : "shm: ok\n", bad);
    return bad != 0;
}
