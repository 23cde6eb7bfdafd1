// Group mode of the training step: between sttode_tgemm_group(1) and sttode_tgemm_group(0) a step's independent launches are queued and
// leave several to a launch.  Each queue lives beside the kernel it launches, as file-local thread_local state: a group belongs to the host
// thread that opened it, and another thread's calls neither see it nor wait for it (no lock is taken: they launch at once).  A queue
// exposes ONE function with one contract: on < 0 forgets what is queued (error paths); then whatever is queued is launched; then
// the queue remembers whether a group is open (on > 0).  Returns 0, or 1 with the error set.  sttode_tgemm_group (train_gemm.hip) owns
// the LDS-tiled, scene-size and split-sum queues itself and is the only caller of these, in this order.
#pragma once
bool stt_tgemm_group_open();   // train_gemm.hip: has the calling thread opened a group?  (for callers whose launches depend on each other)
int stt_ew_group(int on);      // train_ewise.hip: element-wise pieces (ewise_multi_kernel)
int stt_trunk_group(int on);   // train_trunk.hip: the two encoder trunks' fused forwards (ttrunk_fwd2_kernel)
