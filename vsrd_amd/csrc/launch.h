// Host-side launch helpers shared by the two translation units of libvsrd_hip: the dispatch on a launch's number of 64-lane rounds and
// the launch of the residual step's front kernels.  Everything here lives in the kernels' namespace, so split_front.hip (which compiles
// the headers as `vsrd_split`) gets its own copy, bound to its own instantiations of the kernels, from the same source.
#pragma once
#include <cstdio>
#include <cstring>
#include <type_traits>
#include "render_kernels.h"
#include "split_front.h"

namespace vsrd {

// launch(std::integral_constant<int, K>{}) for the K of the list that equals `rounds`; false when the list has no such K.  The list at a
// call site IS the set of instantiations of that site's kernel.
template <int... Ks, class F>
bool for_rounds(int rounds, F&& launch) {
    return ((rounds == Ks ? (launch(std::integral_constant<int, Ks>{}), true) : false) || ...);
}
// launch(std::true_type{}) or launch(std::false_type{})
template <class F>
void for_bool(bool value, F&& launch) {
    if (value) launch(std::true_type{}); else launch(std::false_type{});
}

constexpr size_t kLdsLimit = 160 * 1024;     // gfx950 LDS per CU
constexpr size_t kLdsDefault = 64 * 1024;    // dynamic LDS without opting in

template <typename Kernel>
bool opt_in(Kernel kernel, size_t bytes, bool debug) {
    if (bytes <= kLdsDefault) return true;
    const hipError_t error = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(bytes));
    if (error != hipSuccess && debug) fprintf(stderr, "libvsrd_hip: LDS opt-in of %zu bytes failed: %s\n", bytes, hipGetErrorString(error));
    return error == hipSuccess;
}

// One chunk's front kernel of vsrd_render_residual_step: residual_step_pair_kernel (a ray over two waves; its kFrames form for a batch
// of frames or a frame header) or residual_step_front_kernel (a wave per ray; <2, true> writes the step's samples out).  Returns a code
// of split_front.h.  A kernel's LDS opt-in comes first, then what that kernel cannot do: frames, then sample outputs.
inline int launch_front(const vsrd_split_front::FrontLaunch& a, hipStream_t stream, bool debug) {
    using namespace vsrd_split_front;
    if (a.field_args_bytes != sizeof(FieldArgs) || a.render_args_bytes != sizeof(RenderArgs)) return kUnsupported;
    FieldArgs f;
    RenderArgs c;
    std::memcpy(&f, a.field_args, sizeof f);
    std::memcpy(&c, a.render_args, sizeof c);
    int code = kOk;
    auto launch = [&](auto kernel, int threads, bool refused, auto... frame_header) {
        if (!opt_in(kernel, a.lds_bytes, debug)) { code = kLdsRefused; return; }
        if (refused) { code = kUnsupported; return; }
        hipLaunchKernelGGL(kernel, dim3(a.blocks, a.frames), dim3(threads), a.lds_bytes, stream, f, a.instances, a.images, c, a.origins, a.directions, a.u_coarse,
                           a.u_fine, a.targets, a.instance_weights, a.loss_scale, a.eikonal_scale, a.eikonal_norm, a.labels, a.box_partials,
                           static_cast<float4*>(a.jets), a.loss_partials, a.seeds, a.masks, a.slots_per_instance, a.first, a.rays, a.accumulate, frame_header...);
    };
    bool known = true;
    if (a.pair) {
        known = for_rounds<2, 4>(a.rounds, [&](auto k) {
            for_bool(a.frames > 1 || a.frame_header, [&](auto frames) {
                launch(residual_step_pair_kernel<decltype(k)::value, decltype(frames)::value>, kPairWaves * kWave, false, static_cast<const FrameHeader*>(a.frame_header));
            });
        });
    } else if (a.rounds == 2 && a.export_samples && a.frames <= 1) {         // vsrd_render_config::out_*: num_samples in (32, 64]
        launch(residual_step_front_kernel<2, true>, kBlockThreads, false);
    } else {
        // (a batch's frames are launches of <= 2048 rays: the pair kernel; the samples are written by the two-round instantiation above)
        known = for_rounds<1, 2, 4>(a.rounds, [&](auto k) { launch(residual_step_front_kernel<decltype(k)::value>, kBlockThreads, a.frames > 1 || a.export_samples); });
    }
    if (!known) return kUnsupported;
    if (code != kOk) return code;
    const hipError_t error = hipGetLastError();
    if (error != hipSuccess && debug) fprintf(stderr, "libvsrd_hip: launch failed: %s\n", hipGetErrorString(error));
    return error == hipSuccess ? kOk : kLaunchFailed;
}

}  // namespace vsrd
