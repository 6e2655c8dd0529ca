// snapshot_blob_check.cpp — the snapshot blob's validator as a stand-alone host program (no HIP, no device), for sanitizer runs:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/snapshot_blob_check.cpp -o snapshot_blob_check
//   ./snapshot_blob_check good.blob [other.blob ...]
// Prints the verdict for every file.  The FIRST file must be valid; every single-byte corruption of its 128-byte header (each byte set
// to each of the 255 other values) is then run through the validator as well, from a heap copy of the exact size, so that a read past
// the end of a blob is an error the sanitizer sees.  Exit status 0 unless the first file is invalid or cannot be read.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../phyx_amd/csrc/snapshot_blob.h"

static bool read_file(const char* path, std::vector<unsigned char>& out)
{
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    unsigned char buf[4096];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    std::fclose(f);
    return true;
}

// from an exactly sized heap block at an odd address offset: no slack behind the blob, and no alignment the validator could lean on
static int check_copy(const std::vector<unsigned char>& blob, char* why, size_t why_cap)
{
    unsigned char* p = static_cast<unsigned char*>(std::malloc(blob.size() + 1));
    if (!p) std::abort();
    std::copy(blob.begin(), blob.end(), p + 1);
    const int st = phx::snap_blob_check(blob.empty() ? nullptr : p + 1, blob.size(), why, why_cap);
    std::free(p);
    return st;
}

int main(int argc, char** argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s good.blob [other.blob ...]\n", argv[0]); return 2; }
    char why[256];
    std::vector<unsigned char> good;
    for (int a = 1; a < argc; ++a) {
        std::vector<unsigned char> blob;
        if (!read_file(argv[a], blob)) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        why[0] = 0;
        const int st = check_copy(blob, why, sizeof why);
        std::printf("%-40s %zu bytes: %s%s\n", argv[a], blob.size(), st == PHX_OK ? "valid" : "INVALID: ", why);
        if (a == 1) {
            if (st != PHX_OK) return 1;
            good = blob;
        }
    }
    long accepted = 0, rejected = 0;
    for (size_t at = 0; at < phx::SNAP_HEADER_BYTES && at < good.size(); ++at)
        for (int v = 0; v < 256; ++v) {
            if (v == good[at]) continue;
            std::vector<unsigned char> bad = good;
            bad[at] = (unsigned char)v;
            (check_copy(bad, why, sizeof why) == PHX_OK ? accepted : rejected)++;
        }
    std::printf("single-byte header corruptions: %ld rejected, %ld accepted\n", rejected, accepted);
    return 0;
}
