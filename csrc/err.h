// The error string of libnos_kernels.so's workload kernels (kernels.hip, norm.hip, attn_f32.hip,
// attn_x3.hip): thread-local, defined in kernels.hip, read by nos_kernels_last_error().
#pragma once
#include <string>

// record `msg` as the calling thread's last error
void nos_kernels_set_error(const std::string& msg);

// 0 when the last launch was accepted; else its hipError_t, with "<what>: <hip's text>" recorded
int nos_kernels_check_launch(const char* what);
