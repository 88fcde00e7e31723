/* Prints the C compiler's layout of hsad_lstm_fused_bwd_rec and hsad_lstm_bwd_rec (include/hsad.h) for tests/test_lstm_bptt_ref_cpu.py,
 * which compares it with the ctypes mirrors in hanabi_sad_amd/_lib.py: per struct "struct <name> <sizeof>", then "<field> <offset> <size>"
 * in declaration order. */
#include <stddef.h>
#include <stdio.h>

#include "hsad.h"

#define F(f) printf(#f " %zu %zu\n", offsetof(hsad_lstm_fused_bwd_rec, f), sizeof(((hsad_lstm_fused_bwd_rec*)0)->f))
#define B(f) printf(#f " %zu %zu\n", offsetof(hsad_lstm_bwd_rec, f), sizeof(((hsad_lstm_bwd_rec*)0)->f))

int main(void) {
  printf("struct hsad_lstm_fused_bwd_rec %zu\n", sizeof(hsad_lstm_fused_bwd_rec));
  F(WhhT_blocked);
  F(WihT_above_blocked);
  F(gates);
  F(cseq);
  F(c_before);
  F(dO);
  F(dG16);
  F(dc_io);
  F(has_next);
  F(xchg);
  F(saved_frag_major);
  F(tail_is_zero);
  F(xout);
  F(dO_stage);
  F(sink_WT);
  F(sink_out16);
  F(sink_mask16);
  F(sink_xout);
  F(sink_outT16);
  F(sink_ldT);
  F(sink_bias_grad);
  F(dGT16);
  F(ldT);
  F(bias_grad0);
  F(bias_grad1);
  F(bias_col_map);
  F(layout_steps);
  F(wide_blocks);
  printf("struct hsad_lstm_bwd_rec %zu\n", sizeof(hsad_lstm_bwd_rec));
  B(gates);
  B(cseq);
  B(c_before);
  B(WhhT_blocked);
  B(dO);
  B(dG16);
  B(dc_io);
  B(has_next);
  B(xchg);
  B(saved_frag_major);
  B(tail_is_zero);
  return 0;
}
