// Stand-alone driver of the JPEG host stage (pigeon_amd/csrc/jpeg_entropy.h) for the host compiler's sanitizers: no HIP, no GPU,
// nothing preloaded.  tests/test_jpeg_host_cpu.py builds it with -fsanitize=address,undefined and feeds it truncated and mutated files.
//
//   jpeg_entropy_main CASES      CASES: a file of records [uint32 little-endian length][that many bytes]
//
// Every record is copied into a heap block of exactly its length and decoded into a heap block of exactly the size its layout needs, so
// a read past the file or a write past the coefficient region is a sanitizer report.  Prints one line per record: "ok H W", "refused
// REASON" or "error CODE".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_entropy.h"

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s CASES\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    for (;;) {
        unsigned char lb[4];
        if (fread(lb, 1, 4, f) != 4) break;
        const size_t len = (size_t)lb[0] | (size_t)lb[1] << 8 | (size_t)lb[2] << 16 | (size_t)lb[3] << 24;
        uint8_t* data = (uint8_t*)malloc(len ? len : 1);
        if (len && fread(data, 1, len, f) != len) { fprintf(stderr, "short record\n"); return 2; }
        pgjpeg::Header h;
        if (pgjpeg::parse_header(data, len, &h) != PG_JPEG_R_OK) {
            printf("refused %d\n", h.reason);
            free(data);
            continue;
        }
        pg_jpeg_item it;
        memset(&it, 0, sizeof(it));
        it.height = h.height; it.width = h.width; it.ncomp = h.ncomp; it.hs = h.hs; it.vs = h.vs;
        pgjpeg::block_grid(it.height, it.width, it.ncomp, it.hs, it.vs, it.bw, it.bh);
        size_t bytes = 0;
        for (int c = 0; c < it.ncomp; ++c) { it.coef_off[c] = bytes; bytes += (size_t)it.bw[c] * it.bh[c] * 128; }
        uint8_t* coef = (uint8_t*)aligned_alloc(16, bytes);
        const int e = pgjpeg::decode_image(data, len, &it, coef, bytes);
        if (e) printf("error %d\n", e);
        else printf("ok %d %d\n", it.height, it.width);
        free(coef);
        free(data);
    }
    fclose(f);
    return 0;
}
