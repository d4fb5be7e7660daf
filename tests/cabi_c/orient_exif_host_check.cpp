// Host memory check of the EXIF orientation reader (csrc/orient_exif.h): a stand-alone program for
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Ico-detr-tensorrt_amd/csrc ...
// Per FILE.jpg argument: the reader on every prefix of the file, the whole file last, each prefix a heap block of exactly
// its length, so that the sanitizer sees any read outside [0, bytes).  Prints `name orientation` per file, then `clean`.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <fstream>
#include <iterator>
#include <vector>

#include "orient_exif.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    std::ifstream in(argv[a], std::ios::binary);
    if (!in) return 2;
    const std::vector<char> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    int whole = 0;
    for (size_t n = 1; n <= file.size(); ++n) {
      unsigned char* block = static_cast<unsigned char*>(malloc(n));
      memcpy(block, file.data(), n);
      whole = orient::exif_orientation(block, (int64_t)n);
      free(block);
      if (whole < 1 || whole > 8) return 3;
    }
    const char* name = strrchr(argv[a], '/');
    printf("%s %d\n", name ? name + 1 : argv[a], whole);
  }
  printf("clean\n");
  return 0;
}
