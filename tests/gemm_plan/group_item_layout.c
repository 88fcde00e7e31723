/* Prints the C compiler's layout of hsad_gemm_group_item (include/hsad.h) for tests/test_gemm_plan_cpu.py, which compares it with the
 * ctypes mirror in tests/gemm_group.py: "sizeof <bytes>", then "<field> <offset> <size>" in declaration order. */
#include <stddef.h>
#include <stdio.h>

#include "hsad.h"

#define FIELD(f) printf(#f " %zu %zu\n", offsetof(hsad_gemm_group_item, f), sizeof(((hsad_gemm_group_item*)0)->f))

int main(void) {
  printf("sizeof %zu\n", sizeof(hsad_gemm_group_item));
  FIELD(A);
  FIELD(B);
  FIELD(C);
  FIELD(row_map);
  FIELD(lda);
  FIELD(ldb);
  FIELD(ldc);
  FIELD(M);
  FIELD(N);
  FIELD(K);
  FIELD(n_out);
  FIELD(split_k);
  FIELD(accumulate);
  return 0;
}
