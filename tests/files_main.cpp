// Stand-alone check of ttcross_amd/csrc/ttx_files.h (host code only): the stream file of the genuine reference read and written
// back, files the reader must refuse, the table of code-object images with the verdicts of devfun_image_plausible, a code-object
// file into memory, and the HDF5 round trip where libhdf5 is found.  One line per case (tests/test_files_cpu.py holds them);
// built plain and with -fsanitize=address,undefined by that test.  Arguments: the directory of the fixtures, a directory to write in.
#include "ttx_files.h"

#include <cstdio>
#include <memory>
#include <string>
#include <vector>

typedef std::vector<unsigned char> Bytes;
static std::string g_tmp;

static Bytes slurp(const std::string &path)
{
    Bytes b; std::string text;
    if (devfun_read_file("slurp", path.c_str(), b, &text)) printf("%s\n", text.c_str());
    return b;
}
static std::string spill(const char *name, const Bytes &b)
{
    const std::string path = g_tmp + "/" + name;
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (!b.empty() && fwrite(b.data(), 1, b.size(), f) != b.size())) printf("cannot write %s\n", path.c_str());
    if (f) fclose(f);
    return path;
}
static void put32(Bytes &b, size_t at, int32_t v) { memcpy(b.data() + at, &v, 4); }
static void put64(Bytes &b, size_t at, uint64_t v) { memcpy(b.data() + at, &v, 8); }
// the message with the path taken out
static std::string anonymous(std::string text, const std::string &path)
{
    for (size_t at; (at = text.find(path)) != std::string::npos;) text.replace(at, path.size(), "FILE");
    return text;
}
// Fortran's e25.17
static std::string e25_17(double v)
{
    char buf[64], out[64];
    snprintf(buf, sizeof buf, "%.16E", v);              // d.ddddddddddddddddE+xx
    const std::string s(buf);
    const size_t e = s.find('E');
    const int ex = atoi(s.c_str() + e + 1) + (v != 0.0);
    snprintf(out, sizeof out, "0.%c%sE%c%02d", s[0], s.substr(2, e - 2).c_str(), ex < 0 ? '-' : '+', ex < 0 ? -ex : ex);
    return std::string(25 - strlen(out), ' ') + out;
}

// ---- the stream file ----------------------------------------------------------------------------------------------------------
static int stream_file(const std::string &golden)
{
    int bad = 0;
    const std::string gold = golden + "/ttio_5.tt";
    std::vector<int32_t> n, r;
    std::vector<double> x;
    std::string text;
    if (ttfile_read(gold.c_str(), n, r, x, &text)) { printf("%s\n", text.c_str()); return 1; }
    // the lines the reference's own dtt_read printed for this file (tests/golden/ref_ttio.f90)
    printf("lm%4d%4d\n", 1, (int)n.size());
    printf("n"); for (int v : n) printf("%4d", v); printf("\n");
    printf("r"); for (int v : r) printf("%4d", v); printf("\n");
    double sum = 0.0;
    size_t at = 0;
    for (size_t b = 0; b < n.size(); b++)
        for (int k = 1; k <= r[b + 1]; k++) for (int j = 1; j <= n[b]; j++) for (int i = 1; i <= r[b]; i++) sum += x[at++] * (i + 2 * j + 3 * k + 4 * (double)(b + 1));
    printf("checksum%s\n", e25_17(sum).c_str());
    const std::string back = g_tmp + "/back.tt";
    const Bytes g = slurp(gold);
    const bool same = ttfile_write(back.c_str(), (int)n.size(), n.data(), r.data(), x.data(), &text) == TTX_OK && slurp(back) == g;
    printf("written back: %s\n", same ? "the bytes of the fixture" : "DIFFERENT");
    bad += !same;

    // files the reader refuses: the fixture cut short, or with one field changed (header 128 bytes, lm at 128, n at 136, r at 156, cores at 180)
    auto refusal = [&](const char *what, const Bytes &b) {
        const std::string path = spill("bad.tt", b);
        std::string why;
        const int rc = ttfile_read(path.c_str(), n, r, x, &why);
        printf("%s: %s \"%s\"\n", what, rc == TTX_EINVAL ? "TTX_EINVAL" : rc == TTX_OK ? "TTX_OK" : "another code", anonymous(why, path).c_str());
        bad += rc != TTX_EINVAL;
    };
    for (size_t cut : {(size_t)0, (size_t)127, (size_t)128, (size_t)135, (size_t)136, (size_t)140, g.size() - 8})
        refusal(("cut at " + std::to_string(cut) + " bytes").c_str(), Bytes(g.begin(), g.begin() + cut));
    struct { const char *what; size_t at; int32_t v; size_t at2; int32_t v2; } edits[] = {
        {"ver(1) = 2", 8, 2, 8, 2}, {"l = 0", 128, 0, 128, 0}, {"m < l", 128, 3, 132, 2}, {"m = 2049", 132, 2049, 132, 2049}, {"n(1) = 0", 136, 0, 136, 0},
        {"n(1) = 32001", 136, 32001, 136, 32001}, {"r(0) = 0", 156, 0, 156, 0}, {"r(1) = 129", 160, 129, 160, 129}};
    { Bytes b = g; b[0] = b[1] = 'X'; refusal("txt = XX", b); }
    for (const auto &e : edits) { Bytes b = g; put32(b, e.at, e.v); put32(b, e.at2, e.v2); refusal(e.what, b); }
    {
        // a header that promises 2048 cores of 128 x 32000 x 128 (8 TB) in a file of 16 KB: refused before anything of that size is asked for
        Bytes b(g.begin(), g.begin() + 136);
        b.resize(136 + 4 * 2048 + 4 * 2049);
        put32(b, 132, 2048);
        for (int k = 0; k < 2048; k++) put32(b, 136 + 4 * (size_t)k, 32000);
        for (int k = 0; k <= 2048; k++) put32(b, 136 + 4 * 2048 + 4 * (size_t)k, 128);
        refusal("2048 cores of 128 x 32000 x 128 promised, none there", b);
    }
    return bad;
}

// ---- code-object images -------------------------------------------------------------------------------------------------------
static void verdict(const char *what, const Bytes &b)
{
    std::unique_ptr<unsigned char[]> exact(new unsigned char[b.size() + (b.empty() ? 1 : 0)]);      // a read past the end is seen by the sanitizer
    if (!b.empty()) memcpy(exact.get(), b.data(), b.size());
    printf("%s: %s\n", what, devfun_image_plausible(exact.get(), b.size()) ? "true" : "false");
}
static Bytes elf(size_t nbytes, uint64_t phoff, int phes, int phn, uint64_t shoff, int shes, int shn)
{
    Bytes b(nbytes, 0);
    memcpy(b.data(), "\177ELF", nbytes < 4 ? nbytes : 4);
    if (nbytes < 64) return b;
    b[4] = 2;
    put64(b, 32, phoff); put64(b, 40, shoff);
    const uint16_t h[4] = {(uint16_t)phes, (uint16_t)phn, (uint16_t)shes, (uint16_t)shn};
    memcpy(b.data() + 54, h, 8);
    return b;
}
static Bytes bundle(uint64_t count, size_t nbytes)
{
    Bytes b(nbytes, 0);
    memcpy(b.data(), "__CLANG_OFFLOAD_BUNDLE__", 24);
    put64(b, 24, count);
    return b;
}
static void images()
{
    verdict("ELF, 63 bytes", elf(63, 0, 0, 0, 0, 0, 0));
    { Bytes b = elf(64, 64, 0, 0, 64, 0, 0); b[4] = 1; verdict("ELF, 64 bytes, class 1", b); }
    verdict("ELF, 64 bytes, both tables empty at 64", elf(64, 64, 0, 0, 64, 0, 0));
    verdict("ELF, phoff = nbytes + 1", elf(64, 65, 0, 0, 64, 0, 0));
    verdict("ELF, 2 program headers of 56 bytes up to the end", elf(176, 64, 56, 2, 64, 0, 0));
    verdict("ELF, 2 program headers of 56 bytes one byte past the end", elf(175, 64, 56, 2, 64, 0, 0));
    verdict("ELF, shoff = nbytes + 1", elf(64, 64, 0, 0, 65, 0, 0));
    verdict("ELF, 3 section headers of 64 bytes up to the end", elf(256, 64, 0, 0, 64, 64, 3));
    verdict("ELF, 3 section headers of 64 bytes one byte past the end", elf(255, 64, 0, 0, 64, 64, 3));
    verdict("ELF, 65535 section headers of 65535 bytes", elf(64, 64, 0, 0, 64, 65535, 65535));
    verdict("bundle, 0 entries", bundle(0, 32));
    verdict("bundle, 1025 entries", bundle(1025, 32));
    verdict("bundle, one entry cut at 23 of its 24 bytes", bundle(1, 32 + 23));
    // one entry: {offset 60, size 16, id length 4} at 32, the id at 56, the code object at 60..76
    auto one = [](uint64_t off, uint64_t size, uint64_t idl) { Bytes b = bundle(1, 76); put64(b, 32, off); put64(b, 40, size); put64(b, 48, idl); return b; };
    verdict("bundle, one complete entry", one(60, 16, 4));
    verdict("bundle, entry offset + size one past the end", one(60, 17, 4));
    verdict("bundle, entry offset past the end", one(77, 0, 4));
    verdict("bundle, id length 2^64 - 1", one(60, 16, ~(uint64_t)0));
    verdict("bundle, id one byte past the end", one(60, 16, 21));
    { Bytes b(23, 0); memcpy(b.data(), "CCOB", 4); verdict("CCOB, 23 bytes", b); b.resize(24); verdict("CCOB, 24 bytes", b); }
    verdict("3 bytes", Bytes{0x12, 0x34, 0x56});
    verdict("no bytes", Bytes());
}

static int code_object_files()
{
    int bad = 0;
    std::string text;
    Bytes b;
    const std::string missing = g_tmp + "/missing.co";
    int rc = devfun_read_file("who", missing.c_str(), b, &text);
    printf("missing file: %d \"%s\"\n", rc == TTX_EINVAL, anonymous(text, missing).c_str());
    const std::string empty = spill("empty.co", Bytes());
    rc = devfun_read_file("who", empty.c_str(), b, &text);
    printf("empty file: %d \"%s\"\n", rc == TTX_EINVAL, anonymous(text, empty).c_str());
    rc = devfun_read_file("who", "", b, &text);
    printf("no path: %d \"%s\"\n", rc == TTX_EINVAL, text.c_str());
    Bytes big(70000);
    for (size_t i = 0; i < big.size(); i++) big[i] = (unsigned char)(i * 2654435761u >> 24);
    rc = devfun_read_file("who", spill("big.co", big).c_str(), b, &text);
    const bool same = rc == TTX_OK && b == big;
    printf("70000 bytes in two chunks: %s\n", same ? "read back equal" : "DIFFERENT");
    bad += !same;
    return bad;
}

static int hdf5()
{
    std::string text;
    if (hdf5_load(&text)) { printf("hdf5: not available\n"); return 0; }
    const std::vector<int32_t> n = {3, 2}, r = {1, 2, 1};
    std::vector<double> x(3 * 2 + 2 * 2);
    for (size_t i = 0; i < x.size(); i++) x[i] = 0.25 * (double)i - 1.0;
    const std::string path = g_tmp + "/t.h5";
    std::vector<int32_t> n2, r2;
    std::vector<double> x2;
    const bool ok = hdf5_write_tt(path.c_str(), 2, n.data(), r.data(), x.data(), &text) == TTX_OK &&
                    hdf5_read_tt(path.c_str(), n2, r2, x2, &text) == TTX_OK && n2 == n && r2 == r && x2 == x;
    printf(ok ? "hdf5: round trip ok\n" : "hdf5: round trip FAILED %s\n", text.c_str());
    return !ok;
}

int main(int argc, char **argv)
{
    if (argc != 3) { printf("usage: files_main <directory of the fixtures> <directory to write in>\n"); return 2; }
    g_tmp = argv[2];
    int bad = stream_file(argv[1]);
    images();
    bad += code_object_files();
    bad += hdf5();
    printf(bad ? "files: %d checks FAILED\n" : "files: ok\n", bad);
    return bad != 0;
}
