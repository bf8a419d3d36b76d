/* Prints the layout the COMPILER gives every argument struct of include/x3d_hip.h:
 *   <struct> <sizeof>
 *   <struct>.<field> <offsetof> <sizeof>
 * tests/test_abi.py compares it with the ctypes classes x3d_tf_amd/hip.py derives from the same header, so the
 * field lists below are written out by hand on purpose: a second opinion that shares nothing with that parser.
 * Host code only: no device code, no HIP runtime. */
#include <cstddef>
#include <cstdio>

#include "x3d_hip.h"

#define S(s) { typedef s T; const char* name = #s; std::printf("%s %zu\n", name, sizeof(T));
#define F(f) std::printf("%s.%s %zu %zu\n", name, #f, offsetof(T, f), sizeof(T::f));
#define E }

int main() {
  S(x3d_bn_fold) F(stats) F(count) F(gamma) F(beta) F(moving_mean) F(moving_var) F(eps) F(momentum) F(update_moving)
    F(scale_shift) F(mean_invstd) E
  S(x3d_bn_eval_item) F(gamma) F(beta) F(moving_mean) F(moving_var) F(scale_shift) F(mean_invstd) F(C) E
  S(x3d_pw_fwd_args) F(x) F(w) F(y) F(stats) F(in_scale_shift) F(in_gate) F(in_act) F(N) F(Cin) F(Cout) F(T) F(H) F(W)
    F(stride) F(dtype) F(w_panel) F(in_add) F(in_add_scale_shift) F(in_store) F(out_scale_shift) F(out_add)
    F(out_add_scale_shift) F(out_act) E
  S(x3d_bn_bwd_fold) F(sums) F(count) F(mean_invstd) F(gamma) F(dgamma) F(dbeta) F(coef_out) E
  S(x3d_pw_dgrad_args) F(g) F(yraw) F(coef) F(w) F(dx) F(epi) F(add) F(braw) F(b_scale_shift) F(gate) F(nc_sums) F(N) F(Cin)
    F(Cout) F(T) F(H) F(W) F(dtype) F(w_panel) F(coef_fold) E
  S(x3d_pw_bwd_args) F(g) F(yraw) F(coef) F(w_panel) F(dx) F(epi) F(add) F(braw) F(b_scale_shift) F(gate) F(nc_sums) F(x)
    F(dw) F(N) F(Cin) F(Cout) F(T) F(H) F(W) F(dtype) F(tail_c) F(tail_r) F(tail_sums_c) F(tail_sums_r) F(rc_panel) F(rc_c0)
    F(rc_sums) F(x_stride) F(xH) F(xW) F(dw_slab) F(dw_slab_parts) F(coef_fold) E
  S(x3d_dw_reduce_job) F(slab) F(dw) F(parts) F(elems) E
  S(x3d_pw_pack_item) F(w) F(fwd_panel) F(dgrad_panel) F(Cout) F(Cin) E
  S(x3d_pw_wgrad_args) F(g) F(yraw) F(coef) F(x) F(in_scale_shift) F(in_gate) F(in_act) F(dw) F(N) F(Cin) F(Cout) F(T) F(H)
    F(W) F(stride) F(dtype) F(dw_slab) F(dw_slab_parts) F(coef_fold) E
  S(x3d_dw3d_fwd_args) F(x) F(w) F(y) F(in_scale_shift) F(in_act) F(stats) F(pool) F(N) F(C) F(T) F(H) F(W) F(stride)
    F(dtype) F(in_bn) E
  S(x3d_dw3d_bwd_args) F(dv) F(braw) F(coef_nc) F(araw) F(a_scale_shift) F(w) F(ga) F(a_sums) F(dw) F(N) F(C) F(T) F(H) F(W)
    F(stride) F(dtype) E
  S(x3d_se_bnb_bwd_args) F(nc_sums) F(pool_sums) F(P) F(b_scale_shift) F(b_mean_invstd) F(gamma_b) F(w1) F(b1) F(w2) F(b2)
    F(gate) F(hidden) F(dw1) F(db1) F(dw2) F(db2) F(dgamma_b) F(dbeta_b) F(coef_nc) F(scratch) F(N) F(C) F(Wd) F(reduce) E
  S(x3d_eval_views_args) F(video) F(out) F(F) F(H) F(W) F(T) F(views) F(crops) F(size) F(mean) F(std) F(dtype) E
  S(x3d_train_clip_args) F(video) F(out) F(F) F(H) F(W) F(T) F(rate) F(start) F(jitter) F(size) F(y0) F(x0) F(flip) F(mean)
    F(std) F(dtype) E
  S(x3d_jpeg_image) F(out) F(data_off) F(coef_off) F(plane_off) F(data_len) F(status) F(height) F(width) F(ncomp) F(hs)
    F(vs) F(bw) F(bh) F(mcux) F(mcuy) F(dc_tbl) F(ac_tbl) F(huff_off) F(restart_interval) F(ecs_off) F(ecs_end) F(qt) E
  S(x3d_jpeg_decode_args) F(data) F(images) F(host_images) F(n) F(scratch) F(scratch_bytes) F(status) E
  return 0;
}
