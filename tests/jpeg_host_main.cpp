// The host half of the JPEG decoder (csrc/jpeg_host.h) as a stand-alone program, for a host compiler's
// sanitizers (tests/test_crosscity.py builds it with -fsanitize=address,undefined and runs it on truncated
// and corrupted files).  Each argument is a file of cases, every case a little-endian uint32 length followed
// by that many bytes of a JPEG stream.  A case is copied into a heap block of exactly its size, and the
// coefficient buffer is a heap block of exactly msl_jpeg_coef_elems elements, so a read or write one byte
// outside either is an AddressSanitizer report.  Exit status 0: every case returned MSL_OK, MSL_ERR_SHAPE or
// MSL_ERR_ARG; 1: a bad status or a bad cases file.  Prints the count of each status.
#include <stdio.h>
#include <stdlib.h>

#include "../maxsquareloss_amd/csrc/jpeg_host.h"

int main(int argc, char** argv) {
  long counts[3] = {0, 0, 0};  // OK, SHAPE, ARG
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[a]);
      return 1;
    }
    for (;;) {
      unsigned char lb[4];
      const size_t got = fread(lb, 1, 4, f);
      if (got == 0) break;
      if (got != 4) return 1;
      const size_t n = (size_t)lb[0] | (size_t)lb[1] << 8 | (size_t)lb[2] << 16 | (size_t)lb[3] << 24;
      uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
      if (!data || fread(data, 1, n, f) != n) return 1;
      msl_jpeg_header h;
      int st = msl::jpeg::info(n ? data : nullptr, n, &h);
      if (st == MSL_OK) {
        const size_t elems = msl::jpeg::coef_elems(h);
        if (msl::jpeg::check_header(h) != MSL_OK || elems == 0 || elems > ((size_t)1 << 26)) return 1;
        int16_t* coef = static_cast<int16_t*>(malloc(elems * sizeof(int16_t)));
        uint16_t* quant = static_cast<uint16_t*>(malloc(256 * sizeof(uint16_t)));
        if (!coef || !quant) return 1;
        msl_jpeg_header h2;
        st = msl::jpeg::entropy_decode(data, n, &h2, coef, elems, quant);
        if (st == MSL_OK && msl::jpeg::check_header(h2) != MSL_OK) return 1;
        free(coef);
        free(quant);
      }
      free(data);
      if (st != MSL_OK && st != MSL_ERR_SHAPE && st != MSL_ERR_ARG) {
        fprintf(stderr, "status %d\n", st);
        return 1;
      }
      ++counts[st == MSL_OK ? 0 : st == MSL_ERR_SHAPE ? 1 : 2];
    }
    fclose(f);
  }
  printf("ok %ld shape %ld arg %ld\n", counts[0], counts[1], counts[2]);
  return 0;
}
