// ttx_files.h -- the host side of the file formats (host only: no HIP and no engine in here): the check of a code-object image
// before the runtime's loader sees it, a code-object file into memory, the reference's stream file of a tensor train
// (lib/ttio.f90) and its HDF5 layout (lib/utils.f90).  A train is d mode sizes n, d + 1 ranks r and the cores one after the
// other, core k as the column-major (r(k-1), n(k), r(k)).  Every function returns a TTX_* code and, with a failure, the message
// in *errtext; the entries of ttx_engine.hip hand it on.  tests/files_main.cpp runs all of it on the CPU.
#pragma once
#include <cerrno>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <dlfcn.h>

#include "../../include/ttx.h"

inline int files_refuse(std::string *errtext, const std::string &text) { *errtext = text; return TTX_EINVAL; }

// what hipModuleLoadData accepts: a code-object ELF, or the (plain or compressed) offload bundle of hipcc --genco.  Anything else
// is refused here, so that arbitrary bytes never reach the runtime's loader
inline bool devfun_image_plausible(const unsigned char *p, size_t nbytes)
{
    static const char bundle[] = "__CLANG_OFFLOAD_BUNDLE__";
    const size_t bl = sizeof(bundle) - 1;
    auto u64 = [&](size_t at) { uint64_t v; memcpy(&v, p + at, 8); return v; };
    if (nbytes >= 64 && memcmp(p, "\177ELF", 4) == 0) {
        // ELF64 header: program and section header tables inside the image
        if (p[4] != 2) return false;
        uint16_t phes, phn, shes, shn;
        memcpy(&phes, p + 54, 2); memcpy(&phn, p + 56, 2); memcpy(&shes, p + 58, 2); memcpy(&shn, p + 60, 2);
        const uint64_t phoff = u64(32), shoff = u64(40);
        return phoff <= nbytes && (uint64_t)phes * phn <= nbytes - phoff && shoff <= nbytes && (uint64_t)shes * shn <= nbytes - shoff;
    }
    if (nbytes >= bl + 8 && memcmp(p, bundle, bl) == 0) {
        // uncompressed bundle: entry count, then per entry {offset, size, id length, id}; every entry inside the image
        const uint64_t ne = u64(bl);
        if (ne == 0 || ne > 1024) return false;
        size_t at = bl + 8;
        for (uint64_t i = 0; i < ne; i++) {
            if (at + 24 > nbytes) return false;
            const uint64_t off = u64(at), sz = u64(at + 8), idl = u64(at + 16);
            if (off > nbytes || sz > nbytes - off || idl > nbytes - at - 24) return false;
            at += 24 + (size_t)idl;
        }
        return true;
    }
    return nbytes >= 24 && memcmp(p, "CCOB", 4) == 0;
}
// a code object file into memory; `who` names the entry in the messages
inline int devfun_read_file(const char *who, const char *path, std::vector<unsigned char> &buf, std::string *errtext)
{
    if (!path || !*path) return files_refuse(errtext, std::string(who) + ": path missing");
    FILE *fp = fopen(path, "rb");
    if (!fp) return files_refuse(errtext, std::string(who) + ": cannot read " + path + ": " + strerror(errno));
    unsigned char chunk[65536];
    size_t got;
    while ((got = fread(chunk, 1, sizeof chunk, fp)) > 0) {
        buf.insert(buf.end(), chunk, chunk + got);
        if (buf.size() > ((size_t)1 << 30)) break;
    }
    const bool bad = ferror(fp) != 0;
    fclose(fp);
    if (bad) return files_refuse(errtext, std::string(who) + ": cannot read " + path);
    if (buf.empty()) return files_refuse(errtext, std::string(who) + ": " + path + " is empty");
    return TTX_OK;
}

// ---- the stream file ----------------------------------------------------------------------------------------------------------
// lib/ttio.f90:10-17 `tthead`: 'TT      ', ver(2)=(1,0), inf(4)=(tt_size,0,0,0), comment*64, i(8) with i(1:2)=(l,m); 128 bytes
struct TTFileHead { char txt[8]; int32_t ver[2]; int32_t inf[4]; char comment[64]; int32_t i[8]; };
static_assert(sizeof(TTFileHead) == 128, "stream header is 128 bytes");

// dtt_read (lib/ttio.f90:196-297).  The cores are numbered 1..d here; a file with l > 1 keeps its shape but loses the offset
// (every driver has l = 1)
inline int ttfile_read(const char *path, std::vector<int32_t> &n, std::vector<int32_t> &r, std::vector<double> &cores, std::string *errtext)
{
    FILE *f = fopen(path, "rb");
    if (!f) return files_refuse(errtext, std::string("dtt_read: file not exist: ") + path);  // lib/ttio.f90:210-214
    TTFileHead hd;
    int32_t lm[2];
    auto bad = [&](const char *what) { fclose(f); return files_refuse(errtext, std::string("dtt_read: ") + what + ": " + path); };
    if (fread(&hd, sizeof hd, 1, f) != 1) return bad("error reading header");                // :276-279
    if (hd.txt[0] != 'T' || hd.txt[1] != 'T') return bad("not TT header in file");            // :236-240
    if (hd.ver[0] != 1) return bad("not correct version of TT file");                         // :241-245
    if (fread(lm, sizeof lm, 1, f) != 1) return bad("error reading lm");
    const int l = lm[0], m = lm[1];
    if (l < 1 || m < l || m > 2048) return bad("read strange l,m");                           // :249-251, tt_size
    const int d = m - l + 1;
    n.assign(d, 0); r.assign(d + 1, 0);
    if (fread(n.data(), sizeof(int32_t), d, f) != (size_t)d || fread(r.data(), sizeof(int32_t), d + 1, f) != (size_t)d + 1) return bad("error reading nr");
    size_t sz = 0;
    for (int k = 0; k < d; k++) {
        if (n[k] < 1 || r[k] < 1 || r[k + 1] < 1 || n[k] > 32000 || r[k] > 128 || r[k + 1] > 128) return bad("tt structure has invalid size");
        sz += (size_t)r[k] * n[k] * r[k + 1];
    }
    // the sizes are the file's word: where the file is seen to be shorter than its cores, nothing of that size is allocated
    const long at = ftell(f);
    if (at >= 0 && fseek(f, 0, SEEK_END) == 0) {
        const long end = ftell(f);
        if (end >= at && (size_t)(end - at) / sizeof(double) < sz) return bad("error reading cores");
        if (fseek(f, at, SEEK_SET) != 0) return bad("error reading cores");
    }
    cores.assign(sz, 0.0);
    if (fread(cores.data(), sizeof(double), sz, f) != sz) return bad("error reading cores");
    fclose(f);
    return TTX_OK;
}
// dtt_write (lib/ttio.f90:29-108) of cores 1..d
inline int ttfile_write(const char *path, int d, const int32_t *n, const int32_t *r, const double *cores, std::string *errtext)
{
    size_t sz = 0;
    for (int k = 0; k < d; k++) sz += (size_t)r[k] * n[k] * r[k + 1];
    if (sz == 0) return files_refuse(errtext, "dtt_write: tt structure has invalid size: 0");               // lib/ttio.f90:60-61
    FILE *f = fopen(path, "wb");
    if (!f) return files_refuse(errtext, std::string("dtt_write: error opening file: ") + path);            // :85-88
    TTFileHead hd;
    memset(&hd, 0, sizeof hd);
    memcpy(hd.txt, "TT      ", 8);
    hd.ver[0] = 1; hd.ver[1] = 0; hd.inf[0] = 2048;
    hd.i[0] = 1; hd.i[1] = d;
    const int32_t lm[2] = {1, d};
    bool ok = fwrite(&hd, sizeof hd, 1, f) == 1 && fwrite(lm, sizeof lm, 1, f) == 1;          // :75-76
    ok = ok && fwrite(n, sizeof(int32_t), d, f) == (size_t)d && fwrite(r, sizeof(int32_t), d + 1, f) == (size_t)d + 1;   // :77
    ok = ok && fwrite(cores, sizeof(double), sz, f) == sz;                                    // :78
    ok = (fclose(f) == 0) && ok;
    if (!ok) return files_refuse(errtext, std::string("dtt_write: error writing file: ") + path);
    return TTX_OK;
}

// ---- HDF5 layout of lib/utils.f90:8-57 (save_dtt_to_hdf5): group "TT", datasets "modes" (m ints), "ranks" (m+1 ints),
//      "core_k" (k = 0..m-1) with the Fortran shape (r(k-1), n(k), r(k)) -- i.e. the C dataspace (r(k), n(k), r(k-1)) over the
//      column-major bytes.  libhdf5 is an optional run-time dependency, resolved with dlopen like librccl.
typedef int64_t hid_t_; typedef int herr_t_; typedef unsigned long long hsize_t_;
struct Hdf5Api {
    void *lib = nullptr;
    herr_t_ (*open)() = nullptr;
    hid_t_ (*Fcreate)(const char *, unsigned, hid_t_, hid_t_) = nullptr;
    hid_t_ (*Fopen)(const char *, unsigned, hid_t_) = nullptr;
    herr_t_ (*Fclose)(hid_t_) = nullptr;
    hid_t_ (*Gcreate2)(hid_t_, const char *, hid_t_, hid_t_, hid_t_) = nullptr;
    herr_t_ (*Gclose)(hid_t_) = nullptr;
    hid_t_ (*Screate_simple)(int, const hsize_t_ *, const hsize_t_ *) = nullptr;
    herr_t_ (*Sclose)(hid_t_) = nullptr;
    hid_t_ (*Dcreate2)(hid_t_, const char *, hid_t_, hid_t_, hid_t_, hid_t_, hid_t_) = nullptr;
    hid_t_ (*Dopen2)(hid_t_, const char *, hid_t_) = nullptr;
    hid_t_ (*Dget_space)(hid_t_) = nullptr;
    int (*Sget_simple_extent_dims)(hid_t_, hsize_t_ *, hsize_t_ *) = nullptr;
    herr_t_ (*Dwrite)(hid_t_, hid_t_, hid_t_, hid_t_, hid_t_, const void *) = nullptr;
    herr_t_ (*Dread)(hid_t_, hid_t_, hid_t_, hid_t_, hid_t_, void *) = nullptr;
    herr_t_ (*Dclose)(hid_t_) = nullptr;
    herr_t_ (*Eset_auto2)(hid_t_, void *, void *) = nullptr;
    hid_t_ t_int = -1, t_double = -1;
};
inline Hdf5Api g_h5;
inline int hdf5_load(std::string *errtext)
{
    if (g_h5.lib) return TTX_OK;
    void *L = nullptr;
    for (const char *nm : {"libhdf5.so", "libhdf5.so.103", "/opt/conda/lib/libhdf5.so", "libhdf5_serial.so"}) if ((L = dlopen(nm, RTLD_NOW | RTLD_LOCAL))) break;
    if (!L) { const char *why = dlerror(); return files_refuse(errtext, std::string("save_dtt_to_hdf5: libhdf5.so not found (") + (why ? why : "(null)") + ")"); }
#define H5_(f, name) *(void **)(&g_h5.f) = dlsym(L, name); if (!g_h5.f) return files_refuse(errtext, std::string("libhdf5.so lacks ") + name);
    H5_(open, "H5open") H5_(Fcreate, "H5Fcreate") H5_(Fopen, "H5Fopen") H5_(Fclose, "H5Fclose") H5_(Gcreate2, "H5Gcreate2") H5_(Gclose, "H5Gclose")
    H5_(Screate_simple, "H5Screate_simple") H5_(Sclose, "H5Sclose") H5_(Dcreate2, "H5Dcreate2") H5_(Dopen2, "H5Dopen2") H5_(Dget_space, "H5Dget_space")
    H5_(Sget_simple_extent_dims, "H5Sget_simple_extent_dims") H5_(Dwrite, "H5Dwrite") H5_(Dread, "H5Dread") H5_(Dclose, "H5Dclose") H5_(Eset_auto2, "H5Eset_auto2")
#undef H5_
    if (g_h5.open() < 0) return files_refuse(errtext, "H5open failed");
    hid_t_ *ti = (hid_t_ *)dlsym(L, "H5T_NATIVE_INT_g"), *td = (hid_t_ *)dlsym(L, "H5T_NATIVE_DOUBLE_g");
    if (!ti || !td) return files_refuse(errtext, "libhdf5.so lacks the native type ids");
    g_h5.t_int = *ti; g_h5.t_double = *td;
    g_h5.Eset_auto2(0, nullptr, nullptr);                      // errors are reported through return codes here
    g_h5.lib = L;
    return TTX_OK;
}
inline int hdf5_write_tt(const char *path, int d, const int32_t *n, const int32_t *r, const double *cores, std::string *errtext)
{
    if (int rc = hdf5_load(errtext)) return rc;
    const hid_t_ f = g_h5.Fcreate(path, 2u /* H5F_ACC_TRUNC */, 0, 0);
    if (f < 0) return files_refuse(errtext, std::string("save_dtt_to_hdf5: cannot create ") + path);
    const hid_t_ grp = g_h5.Gcreate2(f, "TT", 0, 0, 0);
    bool ok = grp >= 0;
    auto put = [&](const char *name, int rank, const hsize_t_ *dims, hid_t_ type, const void *buf) {
        const hid_t_ sp = g_h5.Screate_simple(rank, dims, nullptr);
        const hid_t_ ds = (sp >= 0) ? g_h5.Dcreate2(grp, name, type, sp, 0, 0, 0) : -1;
        if (ds < 0 || g_h5.Dwrite(ds, type, 0, 0, 0, buf) < 0) ok = false;
        if (ds >= 0) g_h5.Dclose(ds);
        if (sp >= 0) g_h5.Sclose(sp);
    };
    if (ok) {
        hsize_t_ d1 = (hsize_t_)d;
        put("modes", 1, &d1, g_h5.t_int, n);                                         // utils.f90:25-30
        d1 = (hsize_t_)d + 1;
        put("ranks", 1, &d1, g_h5.t_int, r);                                         // :32-37
        size_t off = 0;
        for (int k = 0; k < d && ok; k++) {                                          // :40-51
            const hsize_t_ d3[3] = {(hsize_t_)r[k + 1], (hsize_t_)n[k], (hsize_t_)r[k]};   // Fortran (r0, n, r1) reversed
            char nm[32]; snprintf(nm, sizeof nm, "core_%d", k);
            put(nm, 3, d3, g_h5.t_double, cores + off);
            off += (size_t)r[k] * n[k] * r[k + 1];
        }
    }
    if (grp >= 0) g_h5.Gclose(grp);
    g_h5.Fclose(f);
    if (!ok) return files_refuse(errtext, std::string("save_dtt_to_hdf5: error writing ") + path);
    return TTX_OK;
}
inline int hdf5_read_tt(const char *path, std::vector<int32_t> &n, std::vector<int32_t> &r, std::vector<double> &cores, std::string *errtext)
{
    if (int rc = hdf5_load(errtext)) return rc;
    const hid_t_ f = g_h5.Fopen(path, 0u /* H5F_ACC_RDONLY */, 0);
    if (f < 0) return files_refuse(errtext, std::string("ttx_read_hdf5: cannot open ") + path);
    auto dims_of = [&](const char *name, int want, hsize_t_ *dims) -> hid_t_ {
        const hid_t_ ds = g_h5.Dopen2(f, name, 0);
        if (ds < 0) return -1;
        const hid_t_ sp = g_h5.Dget_space(ds);
        const int nd = (sp >= 0) ? g_h5.Sget_simple_extent_dims(sp, dims, nullptr) : -1;
        if (sp >= 0) g_h5.Sclose(sp);
        if (nd != want) { g_h5.Dclose(ds); return -1; }
        return ds;
    };
    hsize_t_ dm[3];
    n.clear(); r.clear(); cores.clear();
    bool ok = true;
    hid_t_ ds = dims_of("/TT/modes", 1, dm);
    if (ds < 0) ok = false;
    else { n.resize(dm[0]); ok = g_h5.Dread(ds, g_h5.t_int, 0, 0, 0, n.data()) >= 0; g_h5.Dclose(ds); }
    if (ok) { ds = dims_of("/TT/ranks", 1, dm); if (ds < 0 || dm[0] != n.size() + 1) ok = false; if (ds >= 0) { r.resize(dm[0]); ok = ok && g_h5.Dread(ds, g_h5.t_int, 0, 0, 0, r.data()) >= 0; g_h5.Dclose(ds); } }
    for (size_t k = 0; ok && k < n.size(); k++) {
        char nm[40]; snprintf(nm, sizeof nm, "/TT/core_%zu", k);
        ds = dims_of(nm, 3, dm);
        if (ds < 0 || (int)dm[0] != r[k + 1] || (int)dm[1] != n[k] || (int)dm[2] != r[k]) { ok = false; if (ds >= 0) g_h5.Dclose(ds); break; }
        const size_t off = cores.size(), sz = (size_t)r[k] * n[k] * r[k + 1];
        cores.resize(off + sz);
        ok = g_h5.Dread(ds, g_h5.t_double, 0, 0, 0, cores.data() + off) >= 0;
        g_h5.Dclose(ds);
    }
    g_h5.Fclose(f);
    if (!ok) return files_refuse(errtext, std::string("ttx_read_hdf5: ") + path + " does not hold a tensor train in the layout of lib/utils.f90");
    return TTX_OK;
}
