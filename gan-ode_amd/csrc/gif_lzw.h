// gif_lzw.h -- GIF variable-width LZW, encoder side, on the host.  Plain C++ with no HIP in it, so
// scripts/check_gif_lzw.cpp builds it on its own; api.hip exports it as gode_gif_lzw / gode_gif_lzw_bound.
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>

namespace gif_lzw {

enum { ERR_ARG = -1, ERR_CAP = -2, MAX_CODES = 4096, MAX_BITS = 12 };

// A cap that holds the stream of any n indices: every index emits at most one code of at most 12 bits, a table of 4096 codes
// takes at least 4096 - 258 emitted codes to fill (so a clear code at most every 2048 indices, with room to spare), plus the
// leading clear code, the end code and the last partial byte.
static inline int64_t bound(const int64_t n) {
  if (n < 0) return ERR_ARG;
  return (n + n / 2048 + 4) * 3 / 2 + 2;
}

// LSB-first bit packer that never writes at or behind out + cap
struct BitSink {
  uint8_t* out; int64_t cap, pos; uint32_t acc; int nbits; bool full;
  void put(const uint32_t code, const int width) {
    acc |= code << nbits;
    nbits += width;
    while (nbits >= 8) { byte((uint8_t)(acc & 255u)); acc >>= 8; nbits -= 8; }
  }
  void flush() {
    if (nbits > 0) { byte((uint8_t)(acc & 255u)); acc = 0; nbits = 0; }
  }
  void byte(const uint8_t b) {
    if (pos < cap) out[pos++] = b; else full = true;
  }
};

// (prefix code, next index) -> code, open addressing over 16384 slots (at most 4096 live keys), emptied at every clear code
struct Table {
  enum { SLOTS = 16384 };
  std::vector<int32_t> key; std::vector<uint16_t> val;
  Table() : key(SLOTS), val(SLOTS) {}
  void clear() { memset(key.data(), 0xff, SLOTS * sizeof(int32_t)); }
  static uint32_t hash(const uint32_t k) { return (k * 2654435761u) >> 18; }          // 32 - 14 bits
  // the slot of k: its own, or the empty one where it belongs
  uint32_t find(const int32_t k) const {
    uint32_t s = hash((uint32_t)k);
    while (key[s] != -1 && key[s] != k) s = (s + 1) & (SLOTS - 1);
    return s;
  }
};

// n indices (each below 1 << min_code_size) -> the code stream in out[0 .. return value): a clear code first, widths from
// min_code_size + 1 to 12 bits, a clear code as soon as the table holds 4096 codes, the end code last.  The width grows behind
// the code whose emission lets the DECODER's table reach 1 << width, i.e. when the code this step assigns equals 1 << width.
static inline int64_t encode(const uint8_t* idx, const int64_t n, const int32_t min_code_size, uint8_t* out, const int64_t cap) {
  if (!idx || !out || n < 0 || cap < 0 || min_code_size < 2 || min_code_size > 8) return ERR_ARG;
  const uint32_t clear = 1u << min_code_size, eoi = clear + 1;
  uint32_t next = clear + 2;
  int width = min_code_size + 1;
  BitSink sink = {out, cap, 0, 0, 0, false};
  sink.put(clear, width);
  if (n > 0) {
    Table table;
    table.clear();
    if (idx[0] >= clear) return ERR_ARG;
    uint32_t prefix = idx[0];
    for (int64_t i = 1; i < n; ++i) {
      const uint32_t k = idx[i];
      if (k >= clear) return ERR_ARG;
      const int32_t key = (int32_t)((prefix << 8) | k);
      const uint32_t slot = table.find(key);
      if (table.key[slot] == key) { prefix = table.val[slot]; continue; }
      sink.put(prefix, width);
      if (sink.full) return ERR_CAP;
      table.key[slot] = key;
      table.val[slot] = (uint16_t)next;
      if (next == (1u << width) && width < MAX_BITS) ++width;
      if (++next == MAX_CODES) {
        sink.put(clear, width);
        table.clear();
        next = clear + 2;
        width = min_code_size + 1;
      }
      prefix = k;
    }
    sink.put(prefix, width);
    if (next == (1u << width) && width < MAX_BITS) ++width;       // the decoder adds an entry for this code too
  }
  sink.put(eoi, width);
  sink.flush();
  return sink.full ? (int64_t)ERR_CAP : sink.pos;
}

}  // namespace gif_lzw
