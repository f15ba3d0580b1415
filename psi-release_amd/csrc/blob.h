// A library object's device blob: ONE allocation for every buffer the object owns (host side only).  A buffer is declared ONCE — the pointer
// field it binds, the bytes it reserves, how it starts, and optionally a name — and takes the next 256-byte-aligned offset: the ORDER of the
// declarations is the layout.  psi_blob_realise then allocates, binds the fields and does the uploads, copies and fills in that order.
// The declaring half is plain C++ without a HIP call (tools/blob_host_check.hip drives it against a malloc'ed base).
#pragma once
#include <stddef.h>
#include <string.h>
#include <vector>

struct PsiBuf {
    enum Kind { NONE, HOST, DEVICE, FILL };  // starts uninitialised (a kernel writes it) / as a host array / as a device array / as `fill` bytes
    void *field;                  // address of the pointer field that points at the buffer
    size_t off, reserved, bytes;  // `bytes` of the `reserved` ones are copied or filled; a name's capacity is `bytes`
    const void *src;              // HOST, DEVICE: copied from here (only until psi_blob_realise has done so)
    Kind kind;
    int fill;                     // FILL: 0, or 0xff
    bool null_if_empty;           // the field stays null when bytes == 0
    const char *name;             // the name find() knows it by; nullptr: not exposed
    void or_null() { null_if_empty = true; }
};

struct PsiBlob {
    static constexpr size_t NO_ZERO = ~(size_t)0;
    std::vector<PsiBuf> bufs;
    size_t size = 0;              // bytes declared so far
    size_t zero_begin = NO_ZERO;  // when set: everything from here on is zeroed in one go before the other fills
    template <class T>
    PsiBuf &add(T *&field, size_t reserved, size_t bytes, const void *src, PsiBuf::Kind kind, int fill, const char *name)
    {
        bufs.push_back({&field, size, reserved, bytes, src, kind, fill, false, name});
        size += (reserved + 255) & ~(size_t)255;
        return bufs.back();
    }
    // reserve: where the buffer keeps more room than is copied into it (0: as much as is copied)
    template <class T> PsiBuf &upload(T *&field, const void *src, size_t bytes, size_t reserve = 0)
    {
        return add(field, reserve ? reserve : bytes, bytes, src, PsiBuf::HOST, 0, nullptr);
    }
    template <class T> PsiBuf &copy(T *&field, const void *d_src, size_t bytes, size_t reserve = 0)
    {
        return add(field, reserve ? reserve : bytes, bytes, d_src, PsiBuf::DEVICE, 0, nullptr);
    }
    template <class T> PsiBuf &zero(T *&field, size_t bytes, const char *name = nullptr) { return add(field, bytes, bytes, nullptr, PsiBuf::FILL, 0, name); }
    template <class T> PsiBuf &ones(T *&field, size_t bytes, const char *name = nullptr) { return add(field, bytes, bytes, nullptr, PsiBuf::FILL, 0xff, name); }
    template <class T> PsiBuf &raw(T *&field, size_t bytes) { return add(field, bytes, 0, nullptr, PsiBuf::NONE, 0, nullptr); }
    // base + offset into every field (base null: every field null)
    void bind(char *base) const
    {
        for (const PsiBuf &b : bufs) {
            char *p = base && !(b.null_if_empty && !b.bytes) ? base + b.off : nullptr;
            memcpy(b.field, &p, sizeof(p));                      // (the fields are object pointers of several types: one representation)
        }
    }
    const PsiBuf *find(const char *name) const
    {
        for (const PsiBuf &b : bufs)
            if (b.name && !strcmp(b.name, name)) return &b;
        return nullptr;
    }
};

#include "psi_common.h"

// The blob of T in fresh device memory at *blob, every field bound, every buffer started as declared (synchronous; the caller places its own
// device synchronisations around the call).  On failure nothing stays allocated, *blob and every field are null, HIP's sticky error is
// cleared, the message begins with `who` (the caller's entry point) and the HIP code is returned.
static inline int psi_blob_realise(PsiBlob &T, char **blob, const char *who)
{
    *blob = nullptr;
    const char *what = "hipMalloc";
    hipError_t err = hipMalloc((void **)blob, T.size);
    if (err == hipSuccess && T.zero_begin < T.size) {
        what = "fill";
        err = hipMemset(*blob + T.zero_begin, 0, T.size - T.zero_begin);
    }
    if (err == hipSuccess) T.bind(*blob);
    for (PsiBuf &b : T.bufs) {
        if (err != hipSuccess) break;
        char *p = *blob + b.off;
        const bool zeroed = b.off >= T.zero_begin && b.fill == 0;
        what = b.kind == PsiBuf::FILL ? "fill" : "upload";
        if (!b.bytes || b.kind == PsiBuf::NONE || (b.kind == PsiBuf::FILL && zeroed)) continue;
        if (b.kind == PsiBuf::FILL) err = hipMemset(p, b.fill, b.bytes);
        else err = hipMemcpy(p, b.src, b.bytes, b.kind == PsiBuf::HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice);
    }
    for (PsiBuf &b : T.bufs) b.src = nullptr;                    // the sources do not outlive this call
    if (err == hipSuccess) return 0;
    psi_set_error("%s: %s of the device blob (%zu bytes) failed: %s", who, what, T.size, hipGetErrorString(err));
    if (*blob) (void)hipFree(*blob);
    *blob = nullptr;
    T.bind(nullptr);
    (void)hipGetLastError();
    return (int)err;
}
