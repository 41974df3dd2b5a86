// Stand-alone driver for the host JPEG entropy decoder (witw_amd/csrc_host/jpeg_coef.cpp), progressive files included: built together
// with it under -fsanitize=address,undefined (tests/test_jpeg_progressive_san.py) it shows any read behind the file's bytes and any
// write outside the coefficient / table areas, because all three live in heap blocks of exactly their size.
//   jpeg_prog_check FILE...   ->   one line per file: "<info rc> <decode rc or -> <file>"; exit status 0 unless a file cannot be read
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
int witw_jpeg_info_ex(const uint8_t* data, size_t n, int32_t* info, int flags);
int witw_jpeg_decode_coef_ex(const uint8_t* data, size_t n, int16_t* coef, uint16_t* qt, int flags);
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[a]); return 2; }
        fseek(f, 0, SEEK_END);
        const long size = ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* data = (uint8_t*)malloc(size > 0 ? (size_t)size : 1);
        if (size < 0 || fread(data, 1, (size_t)size, f) != (size_t)size) { fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        fclose(f);
        int32_t* info = (int32_t*)calloc(22, sizeof(int32_t));
        const int rc = witw_jpeg_info_ex(data, (size_t)size, info, 1);
        // (a corrupted frame header may announce up to 65,535 x 65,535 samples: such a file is not decoded here)
        if (rc >= 0 && info[5] > 0 && info[5] <= (1 << 20)) {
            int16_t* coef = (int16_t*)malloc((size_t)info[5] * 64 * sizeof(int16_t));
            uint16_t* qt = (uint16_t*)malloc((size_t)info[2] * 64 * sizeof(uint16_t));
            printf("%d %d %s\n", rc, witw_jpeg_decode_coef_ex(data, (size_t)size, coef, qt, 1), argv[a]);
            free(coef);
            free(qt);
        } else {
            printf("%d - %s\n", rc, argv[a]);
        }
        free(info);
        free(data);
    }
    return 0;
}
