// The two interfaces every FrameGraph node talks to -- the subset the Forward+ path calls.
// Mirrors Runtime/RHI/GraphicsDriver.h:59-224 (IGraphicsDriver) and :226-346 (IGraphicsDriverCommands): same method names,
// argument order and meaning; methods the path never calls (swapchain, vertex buffers, ...) are omitted.  The render-pass
// subset exists for the one full-screen draw in front of the path, LinearizeDepthNode (FrameGraph/LinearizeDepthNode.cpp:22-109).
#pragma once
#include "Types.h"

namespace Sailor::RHI {

class IGraphicsDriver {
public:
    virtual ~IGraphicsDriver() = default;
    virtual void WaitIdle() = 0;                                                                           // :83
    virtual RHICommandListPtr CreateCommandList(bool bIsSecondary = false) = 0;                            // :88
    virtual RHIBufferPtr CreateBuffer(size_t size) = 0;                                                    // :89
    virtual RHIBufferPtr CreateIndirectBuffer(size_t size) = 0;                                            // :91 (here: also keeps the bytes of its last UpdateBuffer on the host)
    virtual RHIShaderPtr CreateShader(const std::string& assetPath, const TVector<std::string>& defines = {}) = 0; // :97 (SPIR-V there; here the asset path + permutation)
    virtual RHITexturePtr CreateTexture(const void* pData, size_t size, ivec2 extent, EFormat format, uint32_t mipLevels = 1) = 0; // :98-108 (pData: level 0)
    virtual RHITexturePtr CreateRenderTarget(ivec2 extent, uint32_t mipLevels, EFormat format) = 0;        // :110-117 (filtration, clamping, usage dropped)
    virtual RHICubemapPtr CreateCubemap(ivec2 extent, uint32_t mipLevels, EFormat format) = 0;             // :137-143
    // :119-120 the pool of temporary render targets (ShadowPrepassNode.cpp:227, :285, :357, :360): a released target is handed out again to the next request
    // of its format and extent, so a steady-state frame allocates none
    virtual RHITexturePtr GetOrAddTemporaryRenderTarget(EFormat format, ivec2 extent) = 0;
    virtual void ReleaseTemporaryRenderTarget(RHITexturePtr renderTarget) = 0;
    virtual void SubmitCommandList(RHICommandListPtr commandList) = 0;                                     // :149
    virtual RHIMaterialPtr CreateMaterial(RHIShaderPtr shader) = 0;                                        // :138-141 (vertex layout / topology / render state dropped)
    virtual RHIShaderBindingSetPtr CreateShaderBindings() = 0;                                             // :152
    virtual bool FillShadersLayout(RHIShaderBindingSetPtr& pShaderBindings, const TVector<RHIShaderPtr>& shaders, uint32_t setNum) = 0; // :153
    virtual RHIShaderBindingPtr AddSsboToShaderBindings(RHIShaderBindingSetPtr& pShaderBindings, const std::string& name, size_t elementSize,
                                                        size_t numElements, uint32_t shaderBinding, bool bBindSsboWithOffset = false) = 0; // :154
    virtual RHIShaderBindingPtr AddBufferToShaderBindings(RHIShaderBindingSetPtr& pShaderBindings, const std::string& name, size_t size,
                                                          uint32_t shaderBinding, EShaderBindingType bufferType) = 0;                       // :155
    virtual RHIShaderBindingPtr AddSamplerToShaderBindings(RHIShaderBindingSetPtr& pShaderBindings, const std::string& name, RHITexturePtr texture,
                                                           uint32_t shaderBinding) = 0;                                                     // :156
    virtual RHIShaderBindingPtr AddSamplerToShaderBindings(RHIShaderBindingSetPtr& pShaderBindings, const std::string& name,
                                                           const TVector<RHITexturePtr>& array, uint32_t shaderBinding) = 0;               // :157
    virtual RHIShaderBindingPtr AddStorageImageToShaderBindings(RHIShaderBindingSetPtr& pShaderBindings, const std::string& name, RHITexturePtr texture,
                                                                uint32_t shaderBinding) = 0;                                                // :158
    virtual RHIShaderBindingPtr AddStorageImageToShaderBindings(RHIShaderBindingSetPtr& pShaderBindings, const std::string& name,
                                                                const TVector<RHITexturePtr>& array, uint32_t shaderBinding) = 0;          // :159
    virtual RHIShaderBindingPtr AddShaderBinding(RHIShaderBindingSetPtr& pShaderBindings, const RHIShaderBindingPtr& binding, const std::string& name,
                                                 uint32_t shaderBinding) = 0;                                                               // :160
};

class IGraphicsDriverCommands {
public:
    virtual ~IGraphicsDriverCommands() = default;
    virtual void BeginDebugRegion(RHICommandListPtr cmdList, const std::string& title) = 0; // :238
    virtual void EndDebugRegion(RHICommandListPtr cmdList) = 0;                              // :239
    virtual void ImageMemoryBarrier(RHICommandListPtr cmd, RHITexturePtr image, EImageLayout newLayout) = 0; // :290
    virtual void ClearImage(RHICommandListPtr cmd, RHITexturePtr dst, float r, float g, float b, float a) = 0;   // :294 (a glm::vec4 there)
    virtual void ClearDepthStencil(RHICommandListPtr cmd, RHITexturePtr dst, float depth, uint32_t stencil) = 0;  // :295 (the canonical fp32 plane has no stencil: the value is dropped)
    virtual bool BlitImage(RHICommandListPtr cmd, RHITexturePtr src, RHITexturePtr dst, ivec4 srcRegionRect, ivec4 dstRegionRect,
                           ETextureFiltration filtration = ETextureFiltration::Linear) = 0; // :293 (equal extents: a copy; scaled: one channel, Nearest)
    virtual void GenerateMipMaps(RHICommandListPtr cmd, RHITexturePtr target) = 0;                                                                  // :296 (cubemaps; 2-D RGBA8 textures)
    virtual void ConvertEquirect2Cubemap(RHICommandListPtr cmd, RHITexturePtr equirect, RHICubemapPtr cubemap) = 0;                                 // :297
    virtual void UpdateShaderBinding(RHICommandListPtr cmd, RHIShaderBindingPtr binding, const void* data, size_t size, size_t variableOffset = 0) = 0; // :303
    virtual void SetMaterialParameter(RHICommandListPtr cmd, RHIShaderBindingSetPtr bindings, const std::string& binding, const std::string& variable,
                                      const void* value, size_t size) = 0;                                                                              // :305
    virtual void UpdateBuffer(RHICommandListPtr cmd, RHIBufferPtr buffer, const void* data, size_t size, size_t offset = 0) = 0;                       // :304
    virtual void BeginRenderPass(RHICommandListPtr cmd, const TVector<RHITexturePtr>& colorAttachments, RHITexturePtr depthStencilAttachment,
                                 bool bClearDepthStencil = false) = 0; // :246-255 (area and clear values dropped; the depth clear is to 0, reversed Z's far plane)
    virtual void BindVertexBuffer(RHICommandListPtr cmd, RHIBufferPtr vertexBuffer, uint32_t offset) = 0;                                           // :316
    virtual void BindIndexBuffer(RHICommandListPtr cmd, RHIBufferPtr indexBuffer, uint32_t offset, bool bUint16InsteadOfUint32 = false) = 0;          // :317
    virtual void PushConstants(RHICommandListPtr cmd, RHIMaterialPtr material, size_t size, const void* ptr) = 0;                                      // :324
    virtual void SetViewport(RHICommandListPtr cmd, float x, float y, float width, float height, ivec2 scissorOffset, ivec2 scissorExtent, float minDepth,
                             float maxDepth) = 0;                                                                                                          // :320 (the scissor is what the path reads)
    virtual void EndRenderPass(RHICommandListPtr cmd) = 0;                                                                                          // :273
    virtual void BindMaterial(RHICommandListPtr cmd, RHIMaterialPtr material) = 0;                                                                  // :276
    virtual void BindShaderBindings(RHICommandListPtr cmd, RHIMaterialPtr material, const TVector<RHIShaderBindingSetPtr>& bindings) = 0;           // :282
    virtual void DrawIndexed(RHICommandListPtr cmd, uint32_t indexCount, uint32_t instanceCount, uint32_t firstIndex, uint32_t vertexOffset,
                             uint32_t firstInstance) = 0;                                                                                           // :285
    virtual void DrawIndexedIndirect(RHICommandListPtr cmd, RHIBufferPtr buffer, size_t offset, uint32_t drawCount, uint32_t stride) = 0;                // :323
    // the recorded form of IGraphicsDriver::CopyBuffer_Immediate (:192).  Not in the reference's command interface: its nodes refill their per-instance SSBO
    // from host arrays (UpdateShaderBinding); the mirror's scene data is device-resident, so the refill is a device copy
    virtual void CopyBuffer(RHICommandListPtr cmd, RHIBufferPtr src, RHIBufferPtr dst, size_t size, size_t srcOffset = 0, size_t dstOffset = 0) = 0;
    // Two more commands the reference's interface does not have, both for ShadowPrepassNode and for the same reason as CopyBuffer: where the reference fills
    // the pass's per-instance SSBO from host arrays (ShadowPrepassNode.cpp:155-201, UpdateShaderBinding), the mirror's instances are device-resident and the
    // runs are gathered on the device from the passes' bitmasks (sailor_hip_shadow_gather_instances_batched).  One job = one run: the bits [begin, end) of the
    // mask that starts `maskOffset` bytes into `masks`, its matrices written from record `dstFirst` of `dst` on, at most `capacity` of them.
    struct ShadowGatherRun { size_t m_maskOffset = 0; uint32_t m_begin = 0, m_end = 0, m_dstFirst = 0, m_capacity = 0; };
    virtual void GatherShadowInstances(RHICommandListPtr cmd, RHIBufferPtr instances, uint32_t numInstances, RHIBufferPtr masks, RHIBufferPtr dst,
                                       const TVector<ShadowGatherRun>& runs) = 0;
    // ... and the caster draws' vertex input: ShadowCaster.shader reads inPosition alone, the backend's rasteriser takes packed vec3 positions
    // (sailor_hip_shadow_extract_positions): positions[v] = vertices[v].m_position
    virtual void ExtractVertexPositions(RHICommandListPtr cmd, RHIBufferPtr vertices, uint32_t numVertices, RHIBufferPtr positions) = 0;
    virtual void Dispatch(RHICommandListPtr cmd, RHIShaderPtr computeShader, uint32_t groupSizeX, uint32_t groupSizeY, uint32_t groupSizeZ,
                          const TVector<RHIShaderBindingSetPtr>& bindings, const void* pPushConstantsData = nullptr,
                          uint32_t sizePushConstantsData = 0) = 0;                                                                                       // :310-314
};

} // namespace Sailor::RHI
