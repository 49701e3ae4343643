// Host check of csrc/fd_inflate.hip's bounds and termination: the kernel, compiled for the CPU against the SIMT interpreter of
// tests/emu, inflates single-byte mutations of three gzip members (one stored, one fixed, one dynamic) under AddressSanitizer and
// UBSan.  Each file lies alone in heap blocks of exactly its sizes, so a read or a store one byte outside is reported.  For each
// mutation: zlib accepted it and the output equals zlib's, or zlib refused it and the status is nonzero.  Nothing is preloaded.
//
//   python tools/make_fuzz_inflate.py fuzz_inflate.bin
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-strict-aliasing -Itests/emu/include -Ise3_diffusion_amd/csrc -Iinclude -x c++ tools/fuzz_inflate.cpp se3_diffusion_amd/csrc/fd_inflate.hip tests/emu/hipemu.cpp -o fuzz_inflate
//   ./fuzz_inflate fuzz_inflate.bin
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/fd_hip.h"

void fd_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfprintf(stderr, fmt, ap);
  va_end(ap);
  fputc('\n', stderr);
}
void fd_count_launch() {}

namespace {

std::vector<unsigned char> g_file;
size_t g_at = 0;

long word() {
  int32_t v;
  if (g_at + 4 > g_file.size()) { fprintf(stderr, "the input file is cut\n"); exit(2); }
  memcpy(&v, &g_file[g_at], 4);
  g_at += 4;
  return v;
}
std::vector<unsigned char> bytes() {
  const long n = word();
  if (n < 0 || g_at + (size_t)n > g_file.size()) { fprintf(stderr, "the input file is cut\n"); exit(2); }
  std::vector<unsigned char> v(g_file.begin() + g_at, g_file.begin() + g_at + n);
  g_at += n;
  return v;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s streams.bin\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { perror(argv[1]); return 2; }
  unsigned char chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) g_file.insert(g_file.end(), chunk, chunk + n);
  fclose(f);

  long wrong = 0, total = 0, refused = 0;
  const long streams = word();
  for (long s = 0; s < streams; ++s) {
    const std::vector<unsigned char> base = bytes(), text = bytes();
    const long mutations = word();
    for (long m = -1; m < mutations; ++m) {                   // (-1: the stream as it is)
      long pos = 0, value = 0, expect = 1;
      std::vector<unsigned char> other;
      if (m >= 0) {
        pos = word(), value = word(), expect = word();        // expect 0: zlib refuses; 1: the base text; 2: the bytes that follow
        if (expect == 2) other = bytes();
      }
      const long n = (long)base.size();
      unsigned char* in = (unsigned char*)malloc(n);          // exact sizes: the sanitizer sees one byte too far
      memcpy(in, base.data(), n);
      if (m >= 0) in[pos] = (unsigned char)value;
      // the caller's sizing (pdb.inflate): ISIZE, but no more than the stream could fill
      long size = (long)in[n - 4] | (long)in[n - 3] << 8 | (long)in[n - 2] << 16 | (long)in[n - 1] << 24;
      if (size > 1032 * n) size = 1032 * n;
      unsigned char* out = (unsigned char*)malloc(size ? size : 1);
      memset(out, 0xAA, size ? size : 1);
      const long in_off[2] = {0, n}, out_off[2] = {0, size};
      const int kind[1] = {1};
      long status[1] = {-1};
      if (fd_inflate(in, n, in_off, 1, kind, out, size, out_off, 1, status, nullptr) != 0) return 2;
      const std::vector<unsigned char>& want = expect == 2 ? other : text;
      bool ok;
      if (expect == 0) ok = status[0] != 0;
      else ok = status[0] == 0 && size == (long)want.size() && (size == 0 || memcmp(out, want.data(), size) == 0);
      if (!ok) {
        ++wrong;
        fprintf(stderr, "stream %ld, mutation %ld (byte %ld = %ld): zlib %s, status %ld (position %ld, kind %ld)\n", s, m, pos, value,
                expect ? "accepts" : "refuses", status[0], status[0] / 16, status[0] % 16);
      }
      refused += status[0] != 0;
      ++total;
      free(in);
      free(out);
    }
  }
  printf("%ld streams, %ld runs, %ld refused, %ld differ from zlib\n", streams, total, refused, wrong);
  return wrong ? 1 : 0;
}
