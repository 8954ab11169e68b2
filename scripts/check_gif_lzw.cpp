// check_gif_lzw.cpp -- stand-alone check of csrc/gif_lzw.h: encodes streams with gif_lzw::encode, decodes
// them with the textbook GIF LZW decoder below and compares; checks the capacity contract against guard bytes.  Exits non-zero
// on the first mismatch.  Meant to be built with sanitizers on the host:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all scripts/check_gif_lzw.cpp -o check_gif_lzw
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../gan-ode_amd/csrc/gif_lzw.h"

struct Decoded {
  std::vector<uint8_t> data;
  int clears = 0;          // clear codes seen, the leading one included
  int64_t codes = 0;       // data codes since the last clear code
  int eoi_width = 0;       // the width the end code was read at
  bool ok = false;
};

static Decoded decode(const uint8_t* in, const int64_t n, const int mcs) {
  Decoded r;
  const int clear = 1 << mcs, eoi = clear + 1;
  std::vector<int> prefix(4096, -1), first(4096, 0);
  std::vector<uint8_t> last(4096, 0);
  for (int i = 0; i < clear; ++i) { first[i] = i; last[i] = (uint8_t)i; }
  int next = clear + 2, width = mcs + 1, prev = -1;
  uint32_t acc = 0;
  int nbits = 0;
  int64_t pos = 0;
  std::vector<uint8_t> tmp;
  for (;;) {
    while (nbits < width) {
      if (pos >= n) return r;                                    // ran out of bytes before the end code
      acc |= (uint32_t)in[pos++] << nbits;
      nbits += 8;
    }
    const int code = (int)(acc & ((1u << width) - 1));
    acc >>= width;
    nbits -= width;
    if (code == clear) {
      next = clear + 2; width = mcs + 1; prev = -1; r.clears += 1; r.codes = 0;
      continue;
    }
    if (code == eoi) {
      r.eoi_width = width;
      r.ok = pos == n && r.clears >= 1;                          // nothing behind the end code but its own padding bits
      return r;
    }
    if (r.clears == 0) return r;                                 // the stream must open with a clear code
    r.codes += 1;
    int emit = code;
    if (prev < 0) {
      if (code >= clear) return r;
    } else {
      if (code > next || (code == next && next >= 4096)) return r;
      if (next < 4096) {
        prefix[next] = prev;
        first[next] = first[prev];
        last[next] = (uint8_t)(code == next ? first[prev] : first[code]);
        next += 1;
      }
    }
    tmp.clear();
    for (int c = emit; c >= 0; c = c < clear ? -1 : prefix[c]) tmp.push_back(last[c]);
    for (size_t i = tmp.size(); i-- > 0;) r.data.push_back(tmp[i]);
    if (next == (1 << width) && width < 12) width += 1;
    prev = code;
  }
}

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); \
                                             failures += 1; } } while (0)

// round trip at cap = bound, then one byte short: refused, and the guard bytes behind out + cap stay as they were
static Decoded round_trip(const char* name, const std::vector<uint8_t>& idx, const int mcs) {
  const int64_t n = (int64_t)idx.size(), bound = gif_lzw::bound(n);
  std::vector<uint8_t> out((size_t)bound);
  const int64_t got = gif_lzw::encode(idx.data(), n, mcs, out.data(), bound);
  Decoded d;
  CHECK(got > 0 && got <= bound, "%s: encode returned %lld (bound %lld)", name, (long long)got, (long long)bound);
  if (got <= 0) return d;
  d = decode(out.data(), got, mcs);
  CHECK(d.ok, "%s: the stream does not decode", name);
  CHECK(d.data == idx, "%s: decoded %zu indices differ from the %zu encoded", name, d.data.size(), idx.size());
  std::vector<uint8_t> tight((size_t)got - 1 + 8, 0xA5);          // exactly cap bytes, then 8 guard bytes
  const int64_t rc = gif_lzw::encode(idx.data(), n, mcs, tight.data(), got - 1);
  CHECK(rc == gif_lzw::ERR_CAP, "%s: cap one byte short returned %lld", name, (long long)rc);
  for (int i = 0; i < 8; ++i) CHECK(tight[(size_t)got - 1 + i] == 0xA5, "%s: guard byte %d written", name, i);
  std::vector<uint8_t> exact((size_t)got);                        // a heap block of exactly `got` bytes: the sanitizer's guard
  CHECK(gif_lzw::encode(idx.data(), n, mcs, exact.data(), got) == got, "%s: cap == size refused", name);
  return d;
}

int main() {
  uint32_t s = 12345u;
  auto rnd = [&s]() { s = s * 1664525u + 1013904223u; return s >> 8; };

  round_trip("n=1", std::vector<uint8_t>(1, 200), 8);
  round_trip("5000 equal", std::vector<uint8_t>(5000, 7), 8);

  std::vector<uint8_t> big(70000);
  for (auto& v : big) v = (uint8_t)(rnd() & 255u);
  {
    std::vector<uint8_t> out((size_t)gif_lzw::bound(70000));
    const int64_t got = gif_lzw::encode(big.data(), 70000, 8, out.data(), (int64_t)out.size());
    const Decoded d = decode(out.data(), got, 8);
    CHECK(d.ok && d.data == big, "70000 random: round trip");
    CHECK(d.clears >= 2, "70000 random: %d clear codes, the table never filled", d.clears);
    round_trip("70000 random", big, 8);
  }

  std::vector<uint8_t> two(3000);
  for (auto& v : two) v = (uint8_t)(rnd() & 1u);
  round_trip("two-valued, min_code_size 2", two, 2);
  for (auto& v : two) v = (uint8_t)(rnd() & 3u);
  round_trip("four-valued, min_code_size 2 (fills the table)", std::vector<uint8_t>(two), 2);

  // every prefix of a random stream: among them are the ones that end exactly at and one code behind each growth of the code
  // width (the decoder's table reaches 512, 1024, 2048 after data code 255, 767, 1791)
  const int at[6] = {255, 256, 767, 768, 1791, 1792}, want_width[6] = {10, 10, 11, 11, 12, 12};
  bool seen[6] = {false, false, false, false, false, false};
  bool seen_before = false;
  for (int n = 1; n <= 4000; ++n) {
    const Decoded d = round_trip("prefix", std::vector<uint8_t>(big.begin(), big.begin() + n), 8);
    if (d.clears != 1) continue;
    if (d.codes == 254) { seen_before = true; CHECK(d.eoi_width == 9, "254 codes: end code at %d bits", d.eoi_width); }
    for (int k = 0; k < 6; ++k)
      if (d.codes == at[k]) {
        seen[k] = true;
        CHECK(d.eoi_width == want_width[k], "%d codes: end code at %d bits, not %d", at[k], d.eoi_width, want_width[k]);
      }
  }
  CHECK(seen_before, "no prefix with 254 codes");
  for (int k = 0; k < 6; ++k) CHECK(seen[k], "no prefix with %d codes", at[k]);

  // refusals
  uint8_t one = 4, buf[8];
  CHECK(gif_lzw::encode(&one, 1, 2, buf, 8) == gif_lzw::ERR_ARG, "an index the code size cannot hold");
  CHECK(gif_lzw::encode(&one, 1, 1, buf, 8) == gif_lzw::ERR_ARG && gif_lzw::encode(&one, 1, 9, buf, 8) == gif_lzw::ERR_ARG,
        "min_code_size outside [2, 8]");
  CHECK(gif_lzw::encode(nullptr, 1, 8, buf, 8) == gif_lzw::ERR_ARG && gif_lzw::encode(&one, 1, 8, nullptr, 8) == gif_lzw::ERR_ARG,
        "null pointers");
  CHECK(gif_lzw::encode(&one, -1, 8, buf, 8) == gif_lzw::ERR_ARG && gif_lzw::bound(-1) == gif_lzw::ERR_ARG, "n < 0");
  CHECK(gif_lzw::encode(&one, 1, 8, buf, 0) == gif_lzw::ERR_CAP, "cap 0");

  if (failures) { printf("check_gif_lzw: %d failure(s)\n", failures); return 1; }
  printf("check_gif_lzw: ok\n");
  return 0;
}
