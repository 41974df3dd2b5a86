// Stand-alone driver for the host JPEG entropy decoder (witw_amd/csrc_host/jpeg_coef.cpp) with the 4:4:0 opt-in (flag bit 1) beside
// the progressive one (bit 0): built together with it under -fsanitize=address,undefined (tests/test_jpeg_440.py) it shows any read
// behind the file's bytes and any write outside the coefficient, table and plan areas, because all of them live in heap blocks of
// exactly their size.
//   jpeg_440_check FILE...   ->   one line per file: "<info rc> <decode rc or -> <plan rc or -> <file>"; exit status 0 unless a file
//   cannot be read
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

extern "C" {
int witw_jpeg_info_ex(const uint8_t* data, size_t n, int32_t* info, int flags);
int witw_jpeg_decode_coef_ex(const uint8_t* data, size_t n, int16_t* coef, uint16_t* qt, int flags);
long long witw_jpeg_entropy_plan_bytes_ex(const uint8_t* data, size_t n, int flags);
long long witw_jpeg_entropy_plan_ex(const uint8_t* data, size_t n, uint8_t* plan, size_t plan_cap, uint16_t* qt, int flags);
}

int main(int argc, char** argv) {
    const int flags = 3;
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
        const int rc = witw_jpeg_info_ex(data, (size_t)size, info, flags);
        // (a corrupted frame header may announce up to 65,535 x 65,535 samples: such a file is not decoded here)
        if (rc >= 0 && info[5] > 0 && info[5] <= (1 << 20)) {
            int16_t* coef = (int16_t*)malloc((size_t)info[5] * 64 * sizeof(int16_t));
            uint16_t* qt = (uint16_t*)malloc((size_t)info[2] * 64 * sizeof(uint16_t));
            printf("%d %d ", rc, witw_jpeg_decode_coef_ex(data, (size_t)size, coef, qt, flags));
            const long long need = witw_jpeg_entropy_plan_bytes_ex(data, (size_t)size, flags);
            if (need > 0) {
                uint8_t* plan = (uint8_t*)malloc((size_t)need);
                printf("%lld %s\n", witw_jpeg_entropy_plan_ex(data, (size_t)size, plan, (size_t)need, qt, flags), argv[a]);
                free(plan);
            } else {
                printf("- %s\n", argv[a]);
            }
            free(coef);
            free(qt);
        } else {
            printf("%d - - %s\n", rc, argv[a]);
        }
        free(info);
        free(data);
    }
    return 0;
}
