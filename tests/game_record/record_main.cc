// Stand-alone harness for hanabi_sad_amd/csrc/hsad_game_record.h (tests/test_game_record_cpu.py builds it with the sanitizers).
// stdin: one command per line, stdout: one answer line per command.
//   cap P H deck_size max_info colors                 -> L ok bytes
//   hdr <15 ints: version P H colors ranks max_info max_life bomb n_moves n_dealt score lives info end L>
//                                                     -> the 16 packed bytes, then the 15 fields unpacked from them
//   col P H colors p0 p1 p2 p3 p4 uid                 -> gr_uid_to_true gr_uid_from_true (perm entry c = p_c)
//   flag <13 increments>                              -> the flag byte
//   filter <8 filter ints> score lives n_moves end hit -> 0 | 1
//   layout L                                          -> GR_OFF_DECK GR_OFF_MOVES gr_record_bytes(L)
#include <cstdio>
#include <cstring>

#include "hsad_game_record.h"

int main() {
  char cmd[16];
  while (scanf("%15s", cmd) == 1) {
    if (!strcmp(cmd, "cap")) {
      int P, H, deck, mi, C;
      if (scanf("%d %d %d %d %d", &P, &H, &deck, &mi, &C) != 5) return 2;
      const int L = gr_capacity(P, H, deck, mi, C);
      printf("%d %d %d\n", L, gr_capacity_ok(L) ? 1 : 0, gr_record_bytes(L));
    } else if (!strcmp(cmd, "hdr")) {
      int v[15];
      for (int i = 0; i < 15; ++i)
        if (scanf("%d", &v[i]) != 1) return 2;
      const GrHeader h = {v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14]};
      uint8_t b[16];
      memset(b, 0xee, sizeof(b));
      gr_pack_header(h, b);
      for (int i = 0; i < 16; ++i) printf("%d ", b[i]);
      const GrHeader u = gr_unpack_header(b);
      printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", u.version, u.P, u.H, u.colors, u.ranks, u.max_info, u.max_life, u.bomb,
             u.n_moves, u.n_dealt, u.score, u.lives, u.info, u.end, u.capacity);
    } else if (!strcmp(cmd, "col")) {
      int P, H, C, p[5], uid;
      if (scanf("%d %d %d %d %d %d %d %d %d", &P, &H, &C, &p[0], &p[1], &p[2], &p[3], &p[4], &uid) != 9) return 2;
      uint32_t perm = 0;
      for (int c = 0; c < 5; ++c) perm |= (uint32_t)p[c] << (3 * c);
      printf("%d %d\n", gr_uid_to_true(uid, P, H, C, perm), gr_uid_from_true(uid, P, H, C, perm));
    } else if (!strcmp(cmd, "flag")) {
      bh_inc inc = 0;
      for (int k = 0; k < HSAD_BH_NSTAT; ++k) {
        int v;
        if (scanf("%d", &v) != 1) return 2;
        inc |= bh_put(k, v);
      }
      printf("%d\n", (int)gr_flags(inc));
    } else if (!strcmp(cmd, "filter")) {
      int f[8], score, lives, n, end, hit;
      for (int i = 0; i < 8; ++i)
        if (scanf("%d", &f[i]) != 1) return 2;
      if (scanf("%d %d %d %d %d", &score, &lives, &n, &end, &hit) != 5) return 2;
      const hsad_game_filter flt = {f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7]};
      printf("%d\n", gr_filter_pass(flt, score, lives, n, end, hit != 0) ? 1 : 0);
    } else if (!strcmp(cmd, "layout")) {
      int L;
      if (scanf("%d", &L) != 1) return 2;
      printf("%d %d %d\n", (int)GR_OFF_DECK, (int)GR_OFF_MOVES, gr_record_bytes(L));
    } else {
      return 2;
    }
  }
  static_assert(kGrIdentityPerm == 0x4688u, "the identity permutation: entry c = c");
  return 0;
}
