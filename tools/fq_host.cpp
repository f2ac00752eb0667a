// fq_host.cpp — fastf_amd/csrc/fastq_kernels.hpp's per-lane functions compiled for the host: the sequence line of a read ->
// its key string, as the device (DNA form) and the host (escape form) build it, checked on the CPU against the reference's
// get_fastq + substring (tests/test_freq_host.py).
#include "../fastf_amd/csrc/fastq_kernels.hpp"
#include <string.h>

extern "C" {
// text[0, len) = the data from the sequence line's first byte to the end of the file (s = 0).  Writes the key string into out
// (cap >= 1025) and returns its length; *dna = 1 when the read took the DNA form.
int fq_host_key(const unsigned char* text, uint64_t len, uint32_t L_in, char* out, int* dna) {
    const uint32_t L = L_in > FQ_HDR ? FQ_HDR : L_in;
    // the lane's nine aligned words, as the device loads them from its window buffer (bytes past the data: anything)
    unsigned char b[40];
    memset(b, 0xa5, sizeof b);
    memcpy(b, text, len < 36 ? len : 36);
    uint32_t w[9];
    memcpy(w, b, sizeof w);
    const uint64_t key = fq_pack_dna(w, 0, len, L);
    if (key) {
        *dna = 1;
        fq_decode_dna(key, L, out);
        out[L] = 0;
        return (int)L;
    }
    *dna = 0;
    const uint32_t n = fq_escape_len(text, len, L);
    memcpy(out, text, n);
    out[n] = 0;
    return (int)n;
}
// fq_pack_dna at every misalignment: the same bytes starting at offset 0..3 of the lane's first word
uint64_t fq_host_pack(const unsigned char* text, uint64_t len, uint32_t off, uint32_t L) {
    unsigned char b[40];
    memset(b, 0x5a, sizeof b);
    memcpy(b + off, text, len < 36 - off ? len : 36 - off);
    uint32_t w[9];
    memcpy(w, b, sizeof w);
    return fq_pack_dna(w, off, len, L);
}
}
