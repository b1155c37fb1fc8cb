// Runtime/GraphicsDriver/HIP -- the new RHI backend, sibling of Runtime/GraphicsDriver/Vulkan.
// Like `class VulkanGraphicsDriver : public IGraphicsDriver, public IGraphicsDriverCommands`
// (GraphicsDriver/Vulkan/VulkanGraphicsDriver.h:22) one object implements both interfaces.  It owns a SailorHipContext and
// translates recorded Dispatches of the path's shaders into calls of the C-ABI (include/sailor_hip.h):
//   "Shaders/ComputeLightCulling.shader" -> sailor_hip_light_cull        (binding contract: ComputeLightCulling.shader:20-47)
//   "Shaders/Standard.shader"            -> sailor_hip_shade             (binding contract: Standard.shader:180-251)
//   "Shaders/ComputeMeshCulling.shader"  -> sailor_hip_mesh_cull_compact (binding contract: ComputeMeshCulling.shader:37-58;
//                                           sailor_hip_mesh_frustum_cull when no indirect buffer is bound)
//   "Shaders/ComputeDepthHighZ.shader"   -> sailor_hip_hiz_downscale     (binding contract: ComputeDepthHighZ.shader:11-17)
//   "Shaders/ComputeHistogram.shader" / "ComputeAverageLuminance.shader" (EyeAdaptationNode's two Dispatches)
//                                        -> sailor_hip_luminance_histogram / sailor_hip_average_luminance (ComputeHistogram.shader:14-25,
//                                           ComputeAverageLuminance.shader:14-27); the `histogram` SSBO is created with room for the node state
//   "Shaders/ComputeBloomDownscale.shader" / "ComputeBloomUpscale.shader" (BloomNode's 2 (levels - 1) Dispatches)
//                                        -> sailor_hip_bloom_downscale / sailor_hip_bloom_upscale (ComputeBloomDownscale.shader:11-18,
//                                           ComputeBloomUpscale.shader:11-20); the level views of the bloom target and `u_dirt_texture` are found by name
//   "Shaders/ComputeBrdfLut.shader" / "ComputeIrradianceMap.shader" / "ComputeEnvMap_IBL.shader" (EnvironmentNode's one-off Dispatches)
//                                        -> sailor_hip_compute_brdf_lut / _compute_irradiance_map / _prefilter_env_level
// and the one full-screen DRAW in front of the path (6 indices with the material of)
//   "Shaders/LinearizeDepth.shader"      -> sailor_hip_linearize_depth   (binding contract: LinearizeDepth.shader:15-59)
//   "Shaders/Tonemapping.shader" {ACES, UNCHARTED2, LUMINANCE} -> sailor_hip_tonemap (binding contract: Tonemapping.shader:52-59)
//   "Shaders/Blur.shader" {EVSM, HORIZONTAL | VERTICAL} -> sailor_hip_evsm_blur_pass (binding contract: Blur.shader:53-61)
//   "Shaders/Blur.shader" under any define set with RADIAL, or without EVSM -> sailor_hip_blur (binding contract: Blur.shader:54-61: set 1 `data`,
//                                           `colorSampler`; HORIZONTAL / VERTICAL / RADIAL become SAILOR_BLUR_* flags)
//   "Shaders/ChromaticAberation.shader"  -> sailor_hip_chromatic_aberration (binding contract: ChromaticAberation.shader:52-57: set 1 `data`, `colorSampler`)
//   "Shaders/HBAO.shader"                -> sailor_hip_hbao              (binding contract: HBAO.shader:50-60)
//   "Shaders/HBAO_Blur.shader" {VERTICAL | HORIZONTAL, exactly one} -> sailor_hip_hbao_blur_pass (binding contract: HBAO_Blur.shader:54-62)
//   "Shaders/Sky.shader" by define set: {FILL} -> sailor_hip_sky_fill, {} (into a cube face view) -> sailor_hip_sky_env_face, {SUN} -> sailor_hip_sky_sun
//                                           (or sailor_hip_sky_sun_clouds once the cloud march has been recorded into `cloudsSampler`),
//                                           {COMPOSE} -> sailor_hip_sky_compose, {CLOUDS} -> sailor_hip_sky_clouds (binding contract: Sky.shader:104-153);
//                                           every other permutation is created "not ready", never drawn
//   "Shaders/Stars.shader" of a material with EBlendMode::Additive, drawn as DrawIndexed(count, 1, 0, 0, 0) over the star mesh -> sailor_hip_sky_stars
//                                           (binding contract: Stars.shader:13-40, :92-97: set 0 `frameData`, set 1 `cloudsSampler`, push constant `model`)
//   "Shaders/SunShafts.shader" of a material with EBlendMode::Multiply -> sailor_hip_sky_sun_shafts (binding contract: SunShafts.shader:26-72: set 0
//                                           `frameData`, set 1 `data`, `cloudsSampler`) -- both only for a driver that opted in with EnableShader
//   "Shaders/MotionBlur.shader"          -> sailor_hip_motion_blur       (binding contract: MotionBlur.shader:26-58: set 0 `frameData` / `previousFrameData`,
//                                           set 1 `data`, `depthSampler`, `colorSampler`) -- only for a driver that opted in with EnableShader
//   "Shaders/Debug.shader" {} | {AO} | {LIGHT_TILES} | {CASCADES} -> sailor_hip_debug_view (binding contract: Debug.shader:81-113: set 1 `ldrSceneSampler`,
//                                           `linearDepthSampler`, set 2 `lightsGrid`, `culledLights`, `g_aoSampler`) -- likewise opt-in; any other define set is
//                                           created "not ready"
//   "Shaders/Blit.shader" of a material with EBlendMode::AlphaBlending ("Blit Clouds") -> sailor_hip_sky_blit_clouds (binding: `colorSampler`)
// a scaled one-channel BlitImage with Nearest filtration -> sailor_hip_blit_nearest
// a scaled RGBA32F or one-channel BlitImage with Linear filtration -> sailor_hip_blit_linear
// and the depth-only instanced draws of the shadow passes (material of)
//   "Shaders/Standard.shader" drawn with DrawIndexed (RenderSceneNode's batches) -> sailor_hip_surface_begin at the pass's first such draw, sailor_hip_surface_draw
//       per draw, and at EndRenderPass sailor_hip_surface_resolve -> the shade over driver-owned planes -> sailor_hip_surface_composite into the colour attachment
//   "Shaders/Standard.shader" { "ALPHA_CUTOUT" } drawn with DrawIndexed (a Masked batch) -> sailor_hip_surface_draw_masked with `material` and `textureSamplers` of the
//       bound sets; a pass that held one ends with sailor_hip_surface_store_depth into its depth attachment after the composite
//   "Shaders/Standard_glTF.shader", with or without { "ALPHA_CUTOUT" }, drawn with DrawIndexed (a batch of an imported model) -> sailor_hip_surface_draw_gltf; a pass that
//       held one ends with sailor_hip_surface_resolve_gltf (aoIn = `g_aoSampler` of the lights set if bound) -> the shade, reading the driver's aoOut as its ao ->
//       sailor_hip_surface_composite_gltf.  A pass without one records exactly the launches above.
//   the same three, and "Shaders/DepthOnly.shader", drawn with DrawIndexedIndirect (DepthPrepassNode; RenderSceneNode under `GPUCulling: true`) ->
//       sailor_hip_surface_draw_indirect per command: the host's copy of the command from the indirect buffer (CreateIndirectBuffer keeps the bytes of its last
//       UpdateBuffer), instanceCount and firstInstance read on the device.  A pass WITHOUT a colour attachment begins from its depth attachment (or from cleared
//       keys) and ends with sailor_hip_surface_store_depth alone.  Any other shader under DrawIndexedIndirect: SAILOR_HIP_ERR_UNSUPPORTED.
//   all of these over a `textureSamplers` table of which the host knows a texture of more than one level (RHIBuffer::m_hipTextureLevels, RHITexture::GetMipLevels()
//       per descriptor; sailor_rt_set_scene_texture_levels) -> sailor_hip_surface_draw_lod / sailor_hip_surface_draw_indirect_lod per draw, and the pass ends with
//       sailor_hip_surface_resolve_lod -> the shade -> sailor_hip_surface_composite_gltf: every texture() at its implicit level of detail.  Without that knowledge
//       the routes above, launch for launch.
//   GenerateMipMaps of a 2-D R8G8B8A8_SRGB / R8G8B8A8_UNORM texture (CreateTexture with mipLevels > 1: the chain behind level 0) -> sailor_hip_texture_generate_mips
//   "Shaders/Gizmo.shader" of a LineList material drawn with DrawIndexed (DebugContext::DrawDebugMesh inside DebugDrawNode's pass) -> sailor_hip_surface_begin from
//       the pass' depth attachment, sailor_hip_debug_lines_draw, sailor_hip_debug_lines_resolve into the colour and the depth attachment (push constant viewProjection,
//       VertexP3C4 vertices, 32-bit indices)
//   "Shaders/ImGuiUI.shader" of a TriangleList material under AlphaBlending drawn with DrawIndexed (RenderImGuiNode's pass) -> the commands of one render pass are
//       gathered, each with the scissor SetViewport left, and EndRenderPass issues ONE sailor_hip_ui_draw over them into the colour attachment (push constants
//       scale / translate, VertexP2UV2C1 vertices, 16- or 32-bit indices, `sTexture` of the bound set as the SailorTextureDesc): order across commands lives
//       inside the kernel.  The workspace is grown by ReserveUiWorkspace (whoever hands draw data over calls it) or when the pass is recorded, never at submit.
//   "Shaders/ShadowCaster.shader" [EVSM]  -> sailor_hip_raster_depth into the pass' depth attachment, and at EndRenderPass sailor_hip_shadow_resolve
//                                            into its colour attachment (push constant lightMatrix, set 1 `data`, vertex positions, 32-bit indices)
// and for the ShadowPrepass and Clear nodes: GatherShadowInstances -> sailor_hip_shadow_gather_instances_batched (the pass's `data` SSBO from its caster
// bitmasks, in place of the reference's host upload), ExtractVertexPositions -> sailor_hip_shadow_extract_positions, ClearDepthStencil and ClearImage ->
// sailor_hip_buffer_fill_u32 / sailor_hip_buffer_fill_pattern over the target's fp32 channels, GetOrAddTemporaryRenderTarget / ReleaseTemporaryRenderTarget
// (a pool: a steady-state frame allocates nothing)
// and for the ExperimentalParticles node:
//   "Experimental/MeshParticles/ComputeParticles.shader" (Dispatch) -> sailor_hip_particles_update (binding contract: ComputeParticles.shader:29-58: set 0 `data`,
//       `particlesData`, set 1 `frameData`, the 20-byte push constants)
//   "Experimental/MeshParticles/Particle.shader" { "SHADOW_CASTER" } drawn with DrawIndexed into a pass with ONE colour attachment and no depth attachment
//       -> sailor_hip_particles_shadow into that attachment; {} into a colour and a depth attachment -> sailor_hip_particles_draw (binding contract:
//       Particle.shader:48-115: `frameData`, `light`, `lightsMatrices`, `data`, `shadowMapSampler`).  Any other define set is created "not ready".  The
//       lights set's `lightsMatrices` is a host block on this path: its first matrix is staged into a driver-owned device buffer when its bytes change; that buffer
//       and the passes' workspace are reserved while the draw is recorded.
#pragma once
#include <map>
#include <memory>
#include <set>
#include <string>
#include "../../RHI/GraphicsDriver.h"

namespace Sailor::GraphicsDriver::HIP {

class HipGraphicsDriver : public RHI::IGraphicsDriver, public RHI::IGraphicsDriverCommands {
public:
    HipGraphicsDriver(int deviceOrdinal, void* stream, bool ownStream);
    ~HipGraphicsDriver() override;
    int GetStatus() const { return m_status; }
    SailorHipContext* GetContext() const { return m_ctx; }
    int GetLastDispatchStatus() const { return m_lastDispatchStatus; }
    // The debug regions in the order SubmitCommandList EXECUTED their BeginDebugRegion commands since the last ClearExecutedRegions: the order in which the
    // regions' work went onto the stream.  For tests: the mesh cull's kernels are not in the context's launch log, their "GPU Culling" region is here.
    const TVector<std::string>& GetExecutedRegions() const { return m_executedRegions; }
    void ClearExecutedRegions() { m_executedRegions.clear(); }
    // the prepared views of a `light` SSBO: created with it, derived for every slot on (re-)creation (HipGraphicsDriver.cpp)
    bool EnsurePreparedLights(RHI::RHIShaderBindingPtr binding, bool zeroRecords);

    // Opt this driver in to a shader that has an entry point but is not routed by default: "Shaders/MotionBlur.shader", "Shaders/Debug.shader" (the frame's
    // tail), "Shaders/Stars.shader", "Shaders/SunShafts.shader" (the Sky node's star points and sun shafts: the older Sky and clouds tests record a frame
    // without them).  CreateShader
    // marks them ready only afterwards (Debug.shader only under a define set that has an entry point); without the opt-in it behaves as it always did.  As with
    // the Bloom node class, the opt-in exists only because older tests of this mirror use MotionBlur.shader as their example of a shader WITHOUT an entry point
    // (a PostProcess entry that must be created and record nothing); in the engine the backend would simply route both.  false for any other path.
    bool EnableShader(const std::string& assetPath);
    bool ReserveUiWorkspace(uint32_t numTriangles); // the UI pass' workspace, grown outside the submitted commands (see "Shaders/ImGuiUI.shader" above)

    // Frame capture (a test facility; RHIFrameGraph::CaptureNextFrame): ONE recorded command that copies each source, as it is when the command executes,
    // to storage + its offset, on the context's stream.  A device source is copied device to device; a host source (a uniform block's bytes) is taken when
    // the command is RECORDED, as UpdateShaderBinding takes its payload, and uploaded when it executes.  If a light cull of this submit still has its
    // compaction on the second queue, the stream waits for it first (the copy may be of lightsGrid / culledLights); what the frame's own commands do is unchanged.
    struct CaptureCopy { const void* m_device = nullptr; TVector<uint8_t> m_host; size_t m_bytes = 0, m_offset = 0; };
    void RecordCapture(RHI::RHICommandListPtr cmd, void* storage, TVector<CaptureCopy> copies);
    // is the context's stream being captured into a hipGraph?  (-1: cannot tell -- the caller then refuses, as for 1)
    int IsStreamCapturing() const;
    bool IsShaderEnabled(const std::string& assetPath) const { return m_enabledShaders.count(assetPath) != 0; }

    // IGraphicsDriver
    void WaitIdle() override;
    RHI::RHICommandListPtr CreateCommandList(bool bIsSecondary = false) override;
    RHI::RHIBufferPtr CreateBuffer(size_t size) override;
    RHI::RHIBufferPtr CreateIndirectBuffer(size_t size) override;
    RHI::RHIShaderPtr CreateShader(const std::string& assetPath, const TVector<std::string>& defines = {}) override;
    RHI::RHITexturePtr CreateTexture(const void* pData, size_t size, RHI::ivec2 extent, RHI::EFormat format, uint32_t mipLevels = 1) override;
    RHI::RHITexturePtr CreateRenderTarget(RHI::ivec2 extent, uint32_t mipLevels, RHI::EFormat format) override;
    RHI::RHICubemapPtr CreateCubemap(RHI::ivec2 extent, uint32_t mipLevels, RHI::EFormat format) override;
    RHI::RHITexturePtr GetOrAddTemporaryRenderTarget(RHI::EFormat format, RHI::ivec2 extent) override;
    void ReleaseTemporaryRenderTarget(RHI::RHITexturePtr renderTarget) override;
    void SubmitCommandList(RHI::RHICommandListPtr commandList) override;
    RHI::RHIMaterialPtr CreateMaterial(RHI::RHIShaderPtr shader) override;
    RHI::RHIShaderBindingSetPtr CreateShaderBindings() override;
    bool FillShadersLayout(RHI::RHIShaderBindingSetPtr& set, const TVector<RHI::RHIShaderPtr>& shaders, uint32_t setNum) override;
    RHI::RHIShaderBindingPtr AddSsboToShaderBindings(RHI::RHIShaderBindingSetPtr& set, const std::string& name, size_t elementSize, size_t numElements,
                                                     uint32_t shaderBinding, bool bBindSsboWithOffset = false) override;
    RHI::RHIShaderBindingPtr AddBufferToShaderBindings(RHI::RHIShaderBindingSetPtr& set, const std::string& name, size_t size, uint32_t shaderBinding,
                                                       RHI::EShaderBindingType bufferType) override;
    RHI::RHIShaderBindingPtr AddSamplerToShaderBindings(RHI::RHIShaderBindingSetPtr& set, const std::string& name, RHI::RHITexturePtr texture,
                                                        uint32_t shaderBinding) override;
    RHI::RHIShaderBindingPtr AddSamplerToShaderBindings(RHI::RHIShaderBindingSetPtr& set, const std::string& name,
                                                        const TVector<RHI::RHITexturePtr>& array, uint32_t shaderBinding) override;
    RHI::RHIShaderBindingPtr AddStorageImageToShaderBindings(RHI::RHIShaderBindingSetPtr& set, const std::string& name, RHI::RHITexturePtr texture,
                                                             uint32_t shaderBinding) override;
    RHI::RHIShaderBindingPtr AddStorageImageToShaderBindings(RHI::RHIShaderBindingSetPtr& set, const std::string& name,
                                                             const TVector<RHI::RHITexturePtr>& array, uint32_t shaderBinding) override;
    RHI::RHIShaderBindingPtr AddShaderBinding(RHI::RHIShaderBindingSetPtr& set, const RHI::RHIShaderBindingPtr& binding, const std::string& name,
                                              uint32_t shaderBinding) override;
    // Split frame: this driver renders tile-row band `rank` of `worldSize` of every frame.  The per-pixel targets bound afterwards
    // (sceneDepth, surface, radiance) hold the band's framebuffer rows only; `frame.viewportSize` stays the whole frame's.  `ncclComm` (an
    // ncclComm_t of worldSize ranks, may be null until an exchange is wanted) is only used by ExchangeLightLists.
    int SetFrameSplit(int rank, int worldSize, void* ncclComm);
    const SailorBand* GetBand() const { return m_worldSize > 1 ? &m_band : nullptr; }
    // The RCCL step of a split frame: the band's lightsGrid / culledLights of the last light cull -> the reference's global buffers (on every
    // rank), recorded on the driver's stream (sailor_hip_exchange_light_lists).  Buffers: tiles x 8 bytes and (1 + tiles x 128) x 4 bytes.
    int ExchangeLightLists(RHI::RHIBufferPtr bandGrid, RHI::RHIBufferPtr bandCulled, RHI::RHIBufferPtr globalGrid, RHI::RHIBufferPtr globalCulled);
    // wrap memory owned by someone else (a torch tensor in the tests, an engine heap in the real thing)
    RHI::RHIBufferPtr WrapBuffer(void* devicePtr, size_t size);
    RHI::RHITexturePtr WrapTexture(void* devicePtr, RHI::ivec2 extent, RHI::EFormat format);
    RHI::RHICubemapPtr WrapCubemap(void* devicePtr, int size, uint32_t mipLevels, RHI::EFormat format);
    RHI::RHITexturePtr WrapRenderTarget(void* devicePtr, RHI::ivec2 extent, uint32_t mipLevels, RHI::EFormat format); // a mip chain laid out like CreateRenderTarget's

    // IGraphicsDriverCommands
    void BeginDebugRegion(RHI::RHICommandListPtr cmdList, const std::string& title) override;
    void EndDebugRegion(RHI::RHICommandListPtr cmdList) override;
    void ImageMemoryBarrier(RHI::RHICommandListPtr cmd, RHI::RHITexturePtr image, RHI::EImageLayout newLayout) override;
    void ClearImage(RHI::RHICommandListPtr cmd, RHI::RHITexturePtr dst, float r, float g, float b, float a) override;
    void ClearDepthStencil(RHI::RHICommandListPtr cmd, RHI::RHITexturePtr dst, float depth, uint32_t stencil) override;
    void GatherShadowInstances(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr instances, uint32_t numInstances, RHI::RHIBufferPtr masks, RHI::RHIBufferPtr dst,
                               const TVector<ShadowGatherRun>& runs) override;
    void ExtractVertexPositions(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr vertices, uint32_t numVertices, RHI::RHIBufferPtr positions) override;
    bool BlitImage(RHI::RHICommandListPtr cmd, RHI::RHITexturePtr src, RHI::RHITexturePtr dst, RHI::ivec4 srcRegionRect, RHI::ivec4 dstRegionRect,
                   RHI::ETextureFiltration filtration = RHI::ETextureFiltration::Linear) override;
    void GenerateMipMaps(RHI::RHICommandListPtr cmd, RHI::RHITexturePtr target) override;
    void ConvertEquirect2Cubemap(RHI::RHICommandListPtr cmd, RHI::RHITexturePtr equirect, RHI::RHICubemapPtr cubemap) override;
    void UpdateShaderBinding(RHI::RHICommandListPtr cmd, RHI::RHIShaderBindingPtr binding, const void* data, size_t size, size_t variableOffset = 0) override;
    void SetMaterialParameter(RHI::RHICommandListPtr cmd, RHI::RHIShaderBindingSetPtr bindings, const std::string& binding, const std::string& variable,
                              const void* value, size_t size) override;
    void UpdateBuffer(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr buffer, const void* data, size_t size, size_t offset = 0) override;
    void BeginRenderPass(RHI::RHICommandListPtr cmd, const TVector<RHI::RHITexturePtr>& colorAttachments, RHI::RHITexturePtr depthStencilAttachment,
                         bool bClearDepthStencil = false) override;
    void BindVertexBuffer(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr vertexBuffer, uint32_t offset) override;
    void BindIndexBuffer(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr indexBuffer, uint32_t offset, bool bUint16InsteadOfUint32 = false) override;
    void PushConstants(RHI::RHICommandListPtr cmd, RHI::RHIMaterialPtr material, size_t size, const void* ptr) override;
    void SetViewport(RHI::RHICommandListPtr cmd, float x, float y, float width, float height, RHI::ivec2 scissorOffset, RHI::ivec2 scissorExtent, float minDepth,
                     float maxDepth) override;
    void EndRenderPass(RHI::RHICommandListPtr cmd) override;
    void BindMaterial(RHI::RHICommandListPtr cmd, RHI::RHIMaterialPtr material) override;
    void BindShaderBindings(RHI::RHICommandListPtr cmd, RHI::RHIMaterialPtr material, const TVector<RHI::RHIShaderBindingSetPtr>& bindings) override;
    void DrawIndexed(RHI::RHICommandListPtr cmd, uint32_t indexCount, uint32_t instanceCount, uint32_t firstIndex, uint32_t vertexOffset,
                     uint32_t firstInstance) override;
    void DrawIndexedIndirect(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr buffer, size_t offset, uint32_t drawCount, uint32_t stride) override;
    void CopyBuffer(RHI::RHICommandListPtr cmd, RHI::RHIBufferPtr src, RHI::RHIBufferPtr dst, size_t size, size_t srcOffset = 0, size_t dstOffset = 0) override;
    void Dispatch(RHI::RHICommandListPtr cmd, RHI::RHIShaderPtr computeShader, uint32_t groupSizeX, uint32_t groupSizeY, uint32_t groupSizeZ,
                  const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const void* pPushConstantsData = nullptr,
                  uint32_t sizePushConstantsData = 0) override;

private:
    int RecordLightCulling(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    // aoOverride: the occlusion plane the ambient term reads instead of the bound g_aoSampler (behind a pass with glTF draws: RecordSurfaceResolveShade)
    int RecordShade(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const float* aoOverride = nullptr);
    // The surface pass a recorded draw works in: the frame data of set 0, the attachments' extent, the whole-frame band and the workspace's size.
    struct SurfacePass { SailorUboFrameData frame; int W = 0, H = 0; SailorBand band {}; size_t bytes = 0; };
    // the band and the size of the surface workspace of a W x H pass; `create`: m_surfaceWorkspace is (re)created at that size
    int SurfaceWorkspace(int W, int H, bool create, SurfacePass& pass);
    // the buffers a pass resolves and shades into: m_surfacePlanes, m_surfaceRadiance and, with glTF draws, m_surfaceAo and m_surfaceEmissive; out of memory if one fails
    int SurfacePassBuffers(size_t pixels, bool gltf);
    // The layer step of every pass, behind SurfacePassBuffers: resolves m_surfaceWorkspace into the planes and shades them into m_surfaceRadiance.  resolveGltf:
    // nullptr = sailor_hip_surface_resolve; else the caller's choice of sailor_hip_surface_resolve_gltf or _lod, which also writes m_surfaceAo (from g_aoSampler,
    // if bound at the frame's extent) and m_surfaceEmissive, and the shade then reads m_surfaceAo.
    using SurfaceResolveGltf = decltype(&sailor_hip_surface_resolve_gltf);
    int RecordSurfaceResolveShade(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const SurfacePass& pass, SurfaceResolveGltf resolveGltf);
    // Begins (first) or continues the pass for one recorded draw and records the draw.  Checks in this order: the bindings and the draw's own buffers
    // (buffersBound), the frame split, the attachments (needColor: a pass without a colour attachment is refused, else it is a depth-only pass of the depth
    // attachment's extent), the draw's host-side ranges (rangesOk, from surface_draw_desc, which filled the descriptor d).  On `first` the workspace is
    // created and the keys start from the depth attachment, or from cleared keys if clearDepth.  d.primBase is set to the pass's and `issue(pass, d)` calls
    // the C entry; a draw it refuses un-begins the pass (RecordSurfaceEnd then has nothing to resolve), one it records advances the pass's primBase.
    template <typename Issue>
    int RecordSurfacePassDraw(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depth, bool first,
                              bool needColor, bool clearDepth, bool buffersBound, bool rangesOk, SailorSurfaceDraw& d, Issue&& issue);
    int RecordSurfaceDraw(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depth,
                          const RHI::RHIBufferPtr& vertices, const RHI::RHIBufferPtr& indices, bool first, uint32_t drawIndex, uint32_t indexCount,
                          uint32_t instanceCount, uint32_t firstIndex, uint32_t vertexOffset, uint32_t firstInstance, uint32_t flags);
    // one command of DrawIndexedIndirect in the surface pass: `host` is the command as the indirect buffer's host copy holds it, `command` the buffer and the
    // byte offset the kernel reads instanceCount and firstInstance from.  A pass without a colour attachment is a depth-only pass (DepthPrepassNode)
    int RecordSurfaceDrawIndirect(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depth,
                                  const RHI::RHIBufferPtr& vertices, const RHI::RHIBufferPtr& indices, bool first, bool clearDepth, uint32_t drawIndex,
                                  const SailorDrawIndexedIndirectData& host, const RHI::RHIBufferPtr& command, size_t commandOffset, uint32_t flags);
    int RecordSurfaceEndDepthOnly(const RHI::RHITexturePtr& depth);
    // A RenderScene pass whose draws all have z-write off (the Transparent queue), recorded at EndRenderPass: m_transparentLayers times { peel_begin, every
    // draw, peel_commit, the resolve, the shade, the blend onto `color` } and one more { peel_begin, draws, peel_commit } whose count is the overflow.  The
    // depth attachment is read only.  Refused with the unsupported status, before anything is launched: a Multiply draw, a split frame.
    // Under mode 1 (SetTransparentMode) the same pass through the per-pixel fragment buckets: bucket_begin, every draw ONCE, then per layer { bucket_layer, the
    // resolve, the shade, the blend } and bucket_layer(budget) for the overflow.  The refusals come first and are common to both routes.
    int RecordTransparentPass(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depth,
                              const TVector<RHI::RHICommandList::TransparentDraw>& draws);
public:
    // the layer budget of a transparent pass (1 .. TRANSPARENT_MAX_LAYERS; default 4): false, and nothing changed, outside the range
    static constexpr uint32_t TRANSPARENT_MAX_LAYERS = 64;
    bool SetTransparentLayers(uint32_t layers) { if (layers < 1 || layers > TRANSPARENT_MAX_LAYERS) return false; m_transparentLayers = layers; return true; }
    // the route of a transparent pass: 0 = the peel (default), 1 = the buckets; false, and nothing changed, for anything else
    bool SetTransparentMode(int mode) { if (mode != 0 && mode != 1) return false; m_transparentMode = mode; return true; }
    // the overflow of the LAST recorded transparent pass: the pixels that still had a fragment behind the budget's layers (0 if no pass was recorded).  A host
    // read that waits for the stream: for the next frame's start, like sailor_hip_exchange_adapt's status -- it is never part of a recorded frame.
    int TransparentOverflow(uint32_t& outPixels);
private:
    int RecordDebugLines(const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depth, const RHI::RHIBufferPtr& vertices, const RHI::RHIBufferPtr& indices,
                         const TVector<uint8_t>& pushConstants, uint32_t indexCount, uint32_t firstIndex, uint32_t vertexOffset);
    int RecordUi(const RHI::RHITexturePtr& color, const RHI::RHIBufferPtr& vertices, const RHI::RHIBufferPtr& indices, bool bIndexUint16,
                 const TVector<uint8_t>& pushConstants, const RHI::RHITexturePtr& font, const TVector<SailorUiCommand>& uiCommands, const RHI::RHIBufferPtr& dCommands);
    int RecordSurfaceEnd(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depthToStore, bool gltf);
    int RecordBrdfLut(const TVector<RHI::RHIShaderBindingSetPtr>& bindings);
    int RecordIrradianceMap(const TVector<RHI::RHIShaderBindingSetPtr>& bindings);
    int RecordEnvPrefilter(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    int RecordMeshCulling(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc, bool occlusion);
    int RecordDepthHighZ(const TVector<RHI::RHIShaderBindingSetPtr>& bindings);
    int RecordLinearizeDepth(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target);
    int RecordLuminanceHistogram(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    int RecordAverageLuminance(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    int RecordTonemap(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, uint32_t operatorFlags);
    int RecordEvsmBlur(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, bool vertical);
    int RecordHbao(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target);
    int RecordHbaoBlur(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, bool vertical);
    int RecordMotionBlur(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target);
    int RecordDebugView(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, int mode);
    int RecordBlur(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, uint32_t flags);
    int RecordChromaticAberration(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target);
    int RecordSky(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, int permutation);
    int RecordSkyClouds(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target);
    int RecordBlitAlphaBlended(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target);
    int RecordStars(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, const RHI::RHIBufferPtr& vertices,
                    const RHI::RHIBufferPtr& indices, uint32_t count, const TVector<uint8_t>& pc, RHI::EBlendMode blend);
    int RecordSunShafts(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& target, RHI::EBlendMode blend);
    int RecordBloomDownscale(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    int RecordBloomUpscale(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    int RecordParticlesUpdate(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const TVector<uint8_t>& pc);
    // one DrawIndexed of Particle.shader: shadowCaster -> into `color` alone (the node's map); else into `color` and `depth`
    int RecordParticlesDraw(const TVector<RHI::RHIShaderBindingSetPtr>& bindings, const RHI::RHITexturePtr& color, const RHI::RHITexturePtr& depth,
                            const RHI::RHIBufferPtr& vertices, const RHI::RHIBufferPtr& indices, bool shadowCaster, uint32_t indexCount, uint32_t instanceCount,
                            uint32_t firstIndex, uint32_t vertexOffset, uint32_t firstInstance);
    // the passes' keys and matrix 0 of `lightsMatrices` on the device: both reserved when the draw is RECORDED (ReserveParticlesBuffers), never at submit; the
    // matrix is copied again only when the block's bytes differ from the last copy
    void ReserveParticlesBuffers(const RHI::RHITexturePtr& color, const TVector<RHI::RHIShaderBindingSetPtr>& bindings, bool shadowCaster);
    RHI::RHIBufferPtr m_particlesWorkspace, m_particlesLightMatrix;
    float m_particlesLightMatrixCopy[16] = {};
    bool m_particlesLightMatrixValid = false;

    SailorHipContext* m_ctx = nullptr;              // == m_ctxOwner.get(): what the C-ABI calls take
    std::shared_ptr<SailorHipContext> m_ctxOwner;   // destroyed with the last buffer that still refers to it
    int m_status = 0;
    int m_lastDispatchStatus = 0;
    TVector<std::string> m_executedRegions;
    std::set<std::string> m_enabledShaders; // EnableShader
    // SkyNode's m_pCloudsTexture while the last thing recorded into it was the cloud march: the SUN draw that samples it (one material for the clear and the
    // march, SkyNode.cpp:611-642) goes through sailor_hip_sky_sun_clouds then, through sailor_hip_sky_sun otherwise.  Reset by every write (BeforeBufferWrite)
    const void* m_marchedClouds = nullptr;
    RHI::RHIBufferPtr m_cullWorkspace;
    RHI::RHIBufferPtr m_starsWorkspace; // the star draw's per-star pixels and fragments (sailor_hip_sky_stars_workspace_bytes), grown when a larger mesh is drawn
    RHI::RHIBufferPtr m_meshCullWorkspace;
    // the surface pass of the render pass being executed (Standard.shader draws): workspace (keys, descriptors), the planes the resolve writes and the shade
    // reads, the shade's radiance; the running primBase; begun = the first draw's sailor_hip_surface_begin went through
    RHI::RHIBufferPtr m_surfaceWorkspace, m_surfacePlanes, m_surfaceRadiance;
    // behind a pass that recorded a Standard_glTF.shader draw: the occlusion the shade reads (min(g_AO, the occlusion texel)) and the emissive term the
    // composite adds
    RHI::RHIBufferPtr m_surfaceAo, m_surfaceEmissive;
    RHI::RHIBufferPtr m_uiWorkspace;
    uint64_t m_surfacePrimBase = 0;
    bool m_surfaceBegun = false;
    // the transparent pass: the orders each pixel committed last, the layers' counters ([layer] committed pixels, [budget] the overflow) and the budget
    RHI::RHIBufferPtr m_peelLast, m_peelCounts;
    RHI::RHIBufferPtr m_transparentBuckets; // mode 1: sailor_hip_surface_bucket_bytes of the frame under the current budget, (budget + 1) x 8 bytes a pixel
    uint32_t m_transparentLayers = 4, m_peelCountsLayers = 0;
    int m_transparentMode = 0;
    bool m_peelRecorded = false;
    int32_t m_cullW = 0, m_cullH = 0, m_cullLights = 0; // geometry of the last light cull: locates its shading-order hint in the workspace
    bool m_cullOrderValid = false;
    std::map<const void*, RHI::RHIBufferPtr> m_rasterWorkspaces; // depth attachment -> the rasteriser's workspace (coarse depth, mesh box, giants' queue)
    // GetOrAddTemporaryRenderTarget's pool, and GatherShadowInstances' scratch (chunk offsets; one count word per run), grown when a command is RECORDED
    struct TemporaryRenderTarget { RHI::RHITexturePtr m_target; bool m_bInUse = false; };
    TVector<TemporaryRenderTarget> m_temporaryRenderTargets;
    RHI::RHIBufferPtr m_shadowGatherWorkspace, m_shadowGatherCounts;
    uint32_t m_exchangesClipped = 0; // exchanges whose global lists arrived clipped (reported by the exchange after them)
    // Round 4: the light cull stops after its per-tile lists (SAILOR_CULL_DEFER_PACK); the compaction into the node's `lightsGrid` / `culledLights`
    // SSBOs is recorded on a second context (own stream) and runs BESIDE the RenderScene shade, which reads the per-tile lists when the two SSBOs
    // it is handed are the ones this frame's cull owns.  The main stream joins the second one at the end of the submit that recorded the cull.
    SailorHipContext* m_ctxAux = nullptr;
    bool m_packPending = false;
    void BeforeBufferWrite(const void* devicePtr);
    SailorBand m_cullBand {};          // the band the last recorded cull ran on
    const void* m_ownGrid = nullptr;   // the SSBOs the last recorded cull fills
    const void* m_ownCulled = nullptr;
    int m_rank = 0, m_worldSize = 1; // the frame split
    void* m_comm = nullptr;
    SailorBand m_band {};
    int32_t m_splitW = 0, m_splitH = 0; // the frame size m_band was computed for
    RHI::RHIBufferPtr m_exchangeWorkspace;
};

} // namespace Sailor::GraphicsDriver::HIP
