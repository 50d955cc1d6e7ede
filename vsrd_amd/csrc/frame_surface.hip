// Fourth translation unit of libvsrd_hip: vsrd_frame_surface (include/vsrd_hip.h) and its kernel (frame_surface.h); its argument checks
// are api.hip's (host_checks.h).  A unit of its own so that api.hip's code object is what it was without the surface render; the headers' namespace
// is renamed, as in split_front.hip, so that this unit's copies of the kernels they define do not collide with api.hip's at link time.
#include "host_checks.h"
#define vsrd vsrd_surface
#include "frame_surface.h"
#undef vsrd

using namespace vsrd_surface;
using namespace vsrd_host;

extern "C" int32_t vsrd_frame_surface(const vsrd_field* field, const vsrd_render_config* config, const vsrd_frame_surface_config* surface,
                                      const float* camera_positions, const float* ray_directions, const float* light, const float* palette,
                                      const uint8_t* background, uint8_t* converged_bits, uint8_t* shadow_bits, uint8_t* instance, float* range,
                                      uint8_t* colors, float* positions, float* normals, const vsrd_frame_header* frame_header, void* stream) {
    static_assert(kSurfaceHardUnion == VSRD_SURFACE_HARD_UNION && kSurfaceShadows == VSRD_SURFACE_SHADOWS, "frame_surface.h and the ABI agree on the flags");
    static_assert(sizeof(vsrd_frame_header) == sizeof(FrameHeader), "wave.h: FrameHeader is vsrd_frame_header");
    static_assert(kRunPixels == kWave, "a run is one wave's pixels");
    if (!valid_field(field) || !config || !surface || !camera_positions || !ray_directions) return VSRD_E_INVALID_ARGUMENT;
    const int32_t image = image_view_status(surface->num_views, surface->view, surface->height, surface->width, surface->num_iterations);
    if (image == VSRD_E_INVALID_ARGUMENT || (colors != nullptr && (light == nullptr || palette == nullptr))) return VSRD_E_INVALID_ARGUMENT;
    if (image != VSRD_OK) return image;
    if (background != nullptr && surface->background_pixels != static_cast<int64_t>(surface->height) * surface->width) return VSRD_E_INVALID_ARGUMENT;
    Frames frames;
    if (!frames_of(config->num_frames, config->frame_stride, &frames)) return VSRD_E_INVALID_ARGUMENT;
    FieldArgs f;
    f.num_instances = field->num_instances;
    f.inv_t = 1.0f / field->temperature;
    SurfaceArgs a;
    a.view = surface->view; a.height = surface->height; a.width = surface->width; a.num_iterations = surface->num_iterations;
    a.criteria = surface->convergence_criteria; a.bounding_radius = surface->bounding_radius; a.shadow_offset = surface->shadow_offset;
    a.flags = surface->flags; a.alpha = surface->alpha; a.shininess = surface->shininess;
    for (int c = 0; c < 3; ++c) {
        a.background_color[c] = surface->background_color[c];
        a.ambient[c] = surface->material_emission[c] + surface->material_ambient[c] * surface->light_ambient[c];
        a.diffuse[c] = surface->light_diffuse[c];
        a.specular[c] = surface->material_specular[c] * surface->light_specular[c];
    }
    SurfaceBuffers b;
    b.camera_positions = camera_positions; b.directions = ray_directions; b.light = light; b.palette = palette; b.background = background;
    b.converged_bits = converged_bits; b.shadow_bits = shadow_bits; b.instance = instance; b.range = range; b.colors = colors;
    b.positions = positions; b.normals = normals;
    const int waves = kSurfaceThreads / kWave;
    const int want = (image_runs(surface->height, surface->width) + waves - 1) / waves;
    const int blocks = want > kMaxBlocks ? kMaxBlocks : want;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const FrameHeader* header = reinterpret_cast<const FrameHeader*>(frame_header);
    if (field->mlp_weights != nullptr)
        hipLaunchKernelGGL(frame_surface_kernel<true>, dim3(blocks, frames.count), dim3(kSurfaceThreads), 0, s, f, field->instances, field->mlp_weights,
                           config->device_schedule, a, b, frames.stride, header);
    else
        hipLaunchKernelGGL(frame_surface_kernel<false>, dim3(blocks, frames.count), dim3(kSurfaceThreads), 0, s, f, field->instances, field->mlp_weights,
                           config->device_schedule, a, b, frames.stride, header);
    return launch_status();
}
