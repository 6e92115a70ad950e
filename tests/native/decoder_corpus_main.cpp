// Runs the host stages of csrc/jpeg_decode.hip and csrc/png_decode.hip over a corpus written by
//     python tests/jpeg_cases.py --write DIR
// with every buffer a heap allocation of exactly the size the entry point is promised, so that a build with
// -fsanitize=address,undefined (make -C oa-dg_amd/csrc decoder-asan) reports any read or write outside them.
//     decoder_corpus_asan DIR/manifest.txt
// manifest.txt: one "kind path H W" per line, kind = jpeg | png | png16.  The return codes are counted, not judged (the
// suite judges them): exit status 0 means every file was processed and the sanitizers stayed silent.  Host code only: no
// device function is called, no GPU is needed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include "oadg_hip.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s manifest.txt\n", argv[0]);
        return 2;
    }
    FILE* m = fopen(argv[1], "r");
    if (!m) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char kind[16], path[4096];
    int H, W;
    long files = 0;
    std::map<int, long> codes;
    while (fscanf(m, "%15s %4095s %d %d", kind, path, &H, &W) == 4) {
        if (H < 1 || W < 1 || H > 4096 || W > 4096) {
            fprintf(stderr, "bad extent for %s\n", path);
            return 2;
        }
        ++files;
        int h = 0, w = 0;
        if (strcmp(kind, "jpeg") == 0) {
            ++codes[oadg_jpeg_size(path, &h, &w)];
            uint8_t* out = (uint8_t*)malloc((size_t)H * W * 3);
            ++codes[oadg_jpeg_decode_bgr(path, out, H, W)];
            free(out);
            const size_t cap = oadg_jpeg_coef_capacity(H, W);
            int16_t* coef = (int16_t*)malloc(cap * sizeof(int16_t));
            oadg_jpeg_desc* desc = (oadg_jpeg_desc*)malloc(sizeof(oadg_jpeg_desc));
            const int rc = oadg_jpeg_entropy_decode(path, H, W, coef, cap, desc);
            ++codes[rc];
            if ((rc == 0) != (desc->ncomp != 0)) {
                fprintf(stderr, "%s: return code %d with ncomp %d\n", path, rc, desc->ncomp);
                return 1;
            }
            // a capacity that is too small must be refused, not written past
            if (cap > 64) ++codes[oadg_jpeg_entropy_decode(path, H, W, coef + cap - 64, 64, desc)];
            free(coef);
            free(desc);
        } else if (strcmp(kind, "png") == 0 || strcmp(kind, "png16") == 0) {
            ++codes[oadg_png_size(path, &h, &w)];
            uint8_t* out = (uint8_t*)malloc((size_t)H * W * 3);
            ++codes[oadg_png_decode_bgr(path, out, H, W)];
            free(out);
            uint16_t* out16 = (uint16_t*)malloc((size_t)H * W * sizeof(uint16_t));
            ++codes[oadg_png_decode_gray16(path, out16, H, W)];
            free(out16);
        } else {
            fprintf(stderr, "unknown kind %s\n", kind);
            return 2;
        }
    }
    fclose(m);
    printf("%ld files;", files);
    for (const auto& c : codes) printf(" rc %d: %ld", c.first, c.second);
    printf("\n");
    return files ? 0 : 2;
}
