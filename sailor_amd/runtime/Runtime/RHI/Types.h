// Linux-buildable mirror of the slice of Sailor's RHI that the Forward+ lighting path touches.
// Mirrors (signatures, names, argument meaning): Runtime/RHI/Types.h:14-30,751-761,781-799 (RHIResource + TRefPtr aliases,
// UboFrameData), RHI/Buffer.h, RHI/Shader.h, RHI/CommandList.h -- with an `m_hip` member where the reference's classes
// carry `m_vulkan` (RHI/Shader.h:17-27,71-76, RHI/Buffer.h:15-24, RHI/CommandList.h:15-20).
#pragma once
#include <memory>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../../include/sailor_hip.h"

namespace Sailor {

// minimal intrusive pointer (the reference: Memory/RefPtr.hpp, TRefPtr<T> over TRefBase)
class TRefBase {
public:
    virtual ~TRefBase() = default;
    void AddRef() const { m_refs.fetch_add(1, std::memory_order_relaxed); }
    void Release() const { if (m_refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete this; }
private:
    mutable std::atomic<int> m_refs { 0 };
};

template <typename T>
class TRefPtr {
public:
    TRefPtr() = default;
    TRefPtr(T* p) : m_p(p) { if (m_p) m_p->AddRef(); }
    TRefPtr(const TRefPtr& o) : m_p(o.m_p) { if (m_p) m_p->AddRef(); }
    template <typename U> TRefPtr(const TRefPtr<U>& o) : m_p(o.GetRawPtr()) { if (m_p) m_p->AddRef(); }
    TRefPtr(TRefPtr&& o) noexcept : m_p(o.m_p) { o.m_p = nullptr; }
    ~TRefPtr() { if (m_p) m_p->Release(); }
    TRefPtr& operator=(TRefPtr o) { std::swap(m_p, o.m_p); return *this; }
    template <typename... A> static TRefPtr Make(A&&... a) { return TRefPtr(new T(std::forward<A>(a)...)); }
    T* operator->() const { return m_p; }
    T& operator*() const { return *m_p; }
    T* GetRawPtr() const { return m_p; }
    explicit operator bool() const { return m_p != nullptr; }
    bool IsValid() const { return m_p != nullptr; }
    void Clear() { if (m_p) m_p->Release(); m_p = nullptr; }
    template <typename U> TRefPtr<U> DynamicCast() const { return TRefPtr<U>(dynamic_cast<U*>(m_p)); }
private:
    T* m_p = nullptr;
};

template <typename T> using TVector = std::vector<T>;

namespace RHI {

class RHIResource : public TRefBase {};
using RHIResourcePtr = TRefPtr<RHIResource>;

struct ivec2 { int32_t x = 0, y = 0; };
struct ivec4 { int32_t x = 0, y = 0, z = 0, w = 0; };

using UboFrameData = SailorUboFrameData; // RHI/Types.h:751-761
using VertexP2UV2C1 = SailorVertexP2UV2C1; // RHI/Types.h:656-661: m_position, m_uv, m_color (R8G8B8A8_UNORM, Renderer.cpp:78-82): ImDrawVert

// RHI/Buffer.h: a device allocation.  m_hip.m_devicePtr is either owned (created through IGraphicsDriver) or wrapped.
class RHIBuffer : public RHIResource {
public:
    struct { void* m_devicePtr = nullptr; bool m_bOwned = false; } m_hip;
    size_t m_size = 0;
    // an indirect buffer (IGraphicsDriver::CreateIndirectBuffer) keeps the bytes of its last UpdateBuffer, as UBO bindings keep m_hostCopy: DrawIndexedIndirect
    // takes indexCount, firstIndex, vertexOffset and the un-culled instanceCount from them ("the command as the host wrote it", include/sailor_hip.h)
    bool m_bIndirect = false;
    TVector<uint8_t> m_hostCopy;
    // a `textureSamplers` table: RHITexture::GetMipLevels() of every descriptor's texture, a host copy (empty: not known, every texture one level).  The
    // surface pass takes the entry points with the implicit level of detail iff an entry exceeds 1.
    TVector<uint32_t> m_hipTextureLevels;
    ~RHIBuffer() override;
    // The context the allocation belongs to, shared with the driver that made it: a buffer (or a texture / binding holding one) may outlive
    // the driver object, and the context is destroyed by whoever lets go of it last.
    std::shared_ptr<SailorHipContext> m_ctx;
};
using RHIBufferPtr = TRefPtr<RHIBuffer>;

enum class EFormat { R32_SFLOAT, R16_SFLOAT, R32G32B32A32_SFLOAT, R32G32_SFLOAT, R8_UNORM, R8G8B8A8_UNORM, R8G8B8A8_SRGB }; // the 8-bit ones: SkyNode's weather map and noise volumes, material textures
enum class EPrimitiveTopology { TriangleList, LineList }; // RHI/Types.h EPrimitiveTopology, the two the path draws with
enum class EBlendMode { None, Additive, AlphaBlending, Multiply }; // RHI/Types.h EBlendMode; VulkanPipileneStates.cpp:236-254
enum class ETextureFiltration { Nearest, Linear }; // RHI/Types.h ETextureFiltration (Bicubic has no user on the path)
enum class EImageLayout { Undefined, ShaderReadOnlyOptimal, General, ColorAttachmentOptimal, ComputeWrite, TransferSrcOptimal, TransferDstOptimal };

// RHI/Texture.h: here a linear row-major image in device memory (row 0 = top)
class RHITexture : public RHIResource {
public:
    RHIBufferPtr m_buffer;
    ivec2 m_extent;
    EFormat m_format = EFormat::R32_SFLOAT;
    uint32_t m_mipLevels = 1; // a cubemap is 6 faces x m_extent.x^2 texels per level, level-major (include/sailor_hip.h SailorIblDesc)
    bool m_bCubemap = false;
    bool m_bRepeat = true;    // ETextureClamping::Repeat (the TextureAssetInfo default) vs Clamp: read by ConvertEquirect2Cubemap's sampler
    // a mip-level view of a cubemap (RHI/Cubemap.h:24 GetMipLevel): shares m_buffer with its parent
    TRefPtr<RHITexture> m_parent;
    uint32_t m_viewLevel = 0;
    int32_t m_viewFace = -1;  // >= 0: one face of that level (RHI/Cubemap.h GetFace(face, mipLevel), the attachment SkyNode.cpp:771 renders into)
    // HIP backend, EyeAdaptationNode's 1 x 1 average-luminance target only: the node state (include/sailor_hip.h sailor_hip_eye_adaptation_state_size)
    // whose luminance word m_buffer is a view of -- the `histogram` SSBO the target is bound beside (EyeAdaptationNode.cpp:102-108)
    RHIBufferPtr m_hipEyeAdaptationState;
    // RHI::IsDepthFormat(GetFormat()) of the reference: the canonical fp32 plane of a D32_SFLOAT* / D16_UNORM* target remembers that it is one
    // (BlitNode.cpp:67,88 picks the blit's filtration by it)
    bool m_bDepthFormat = false;
    // a volume (sampler3D, SkyNode.cpp:264-339): m_depth slices of m_extent, x fastest.  1 = a plain image
    int32_t m_depth = 1;
    ivec2 GetExtent() const { return m_extent; }
    uint32_t GetMipLevels() const { return m_mipLevels; }
    TRefPtr<RHITexture> GetMipLevel(uint32_t mipLevel) const;
    TRefPtr<RHITexture> GetFace(uint32_t face, uint32_t mipLevel) const;
};
using RHITexturePtr = TRefPtr<RHITexture>;
using RHICubemapPtr = RHITexturePtr; // RHI/Cubemap.h:15: class RHICubemap : public RHITexture

enum class EShaderBindingType { UniformBuffer, StorageBuffer, CombinedImageSampler, StorageImage };

// RHI/ShaderBinding.h: one named resource at one binding slot
class RHIShaderBinding : public RHIResource {
public:
    std::string m_name;
    EShaderBindingType m_type = EShaderBindingType::StorageBuffer;
    uint32_t m_binding = 0;
    RHIBufferPtr m_buffer;              // SSBO / UBO storage
    TVector<RHITexturePtr> m_textures;  // sampler (array)
    TVector<uint8_t> m_hostCopy;        // UBOs keep the last uploaded bytes: the HIP entry points take them by value
    // HIP backend, the `light` SSBO only: the prepared views of its records (sailor_hip_prepare_lights), kept in step by UpdateShaderBinding
    TRefPtr<class RHIBuffer> m_hipPreparedLights;
    int32_t m_hipPreparedCapacity = 0;
    size_t GetBufferOffset() const { return 0; }
};
using RHIShaderBindingPtr = TRefPtr<RHIShaderBinding>;

class RHIShaderBindingSet : public RHIResource {
public:
    RHIShaderBindingPtr GetOrAddShaderBinding(const std::string& name)
    {
        auto it = m_bindings.find(name);
        if (it != m_bindings.end()) return it->second;
        auto b = RHIShaderBindingPtr::Make();
        b->m_name = name;
        m_bindings[name] = b;
        return b;
    }
    RHIShaderBindingPtr Find(const std::string& name) const
    {
        auto it = m_bindings.find(name);
        return it == m_bindings.end() ? RHIShaderBindingPtr() : it->second;
    }
    std::map<std::string, RHIShaderBindingPtr> m_bindings;
    // IGraphicsDriver::FillShadersLayout: the shader whose reflected layout this set follows ("" = none assigned).  The HIP backend has no
    // reflection; it knows the uniform blocks of the shaders it routes by their asset path.
    std::string m_layoutShader;
};
using RHIShaderBindingSetPtr = TRefPtr<RHIShaderBindingSet>;

// RHI/Shader.h: identified by the asset path the reference loads it from (e.g. "Shaders/ComputeLightCulling.shader")
class RHIShader : public RHIResource {
public:
    explicit RHIShader(std::string name, std::vector<std::string> defines = {}) : m_name(std::move(name)), m_defines(std::move(defines)) {}
    std::string m_name;
    std::vector<std::string> m_defines; // the permutation (ShaderCompiler::LoadShader_Immediate(fileId, shader, { "VERTICAL", "EVSM" }), ShadowPrepassNode.cpp:60)
    bool HasDefine(const std::string& d) const { for (auto& x : m_defines) if (x == d) return true; return false; }
    // RHI/Shader.h IsReady(): compiled and usable.  Here: the backend has an entry point for it (HipGraphicsDriver::CreateShader)
    bool m_bIsReady = true;
    bool IsReady() const { return m_bIsReady; }
};
using RHIShaderPtr = TRefPtr<RHIShader>;

// RHI/Material.h: for this path a material is its shader (render state, vertex layout and topology have no meaning for a
// full-screen pass executed as a compute kernel)
class RHIMaterial : public RHIResource {
public:
    explicit RHIMaterial(RHIShaderPtr shader) : m_shader(std::move(shader)) {}
    RHIShaderPtr m_shader;
    // RenderState::m_blendMode, the one member of the render state a full-screen pass executed as a kernel still needs: "Blit Clouds" is Blit.shader
    // under AlphaBlending (SkyNode.cpp:476-480)
    EBlendMode m_blendMode = EBlendMode::None;
    // RenderState::m_cullMode == ECullMode::None (a glTF doubleSided material); otherwise back faces are culled.  Read by the draws of Standard.shader only.
    bool m_bDoubleSided = false;
    // RenderState::m_bEnableZWrite.  false = a material of the Transparent queue (ModelImporter.cpp:213-229: depth test on, z-write off): its draws of
    // Standard.shader / Standard_glTF.shader are blended in primitive order under m_blendMode, and the depth attachment is read only
    bool m_bZWrite = true;
    // the topology the material's pipeline was created with (CreateMaterial(vertexDescription, topology, ...)): LineList for DebugContext's Gizmo material
    EPrimitiveTopology m_topology = EPrimitiveTopology::TriangleList;
};
using RHIMaterialPtr = TRefPtr<RHIMaterial>;

// RHI/CommandList.h: recorded work, executed at SubmitCommandList (record-then-submit, RHI/GraphicsDriver.h:149)
class RHICommandList : public RHIResource {
public:
    struct { TVector<std::function<int()>> m_commands; } m_hip;
    TVector<std::string> m_debugRegions; // names seen by BeginDebugRegion, for tests
    // state of the render pass being recorded (BeginRenderPass .. EndRenderPass)
    TVector<TRefPtr<class RHITexture>> m_colorAttachments;
    TRefPtr<class RHITexture> m_depthAttachment;
    TRefPtr<class RHIBuffer> m_vertexBuffer, m_indexBuffer;   // BindVertexBuffer / BindIndexBuffer
    TVector<uint8_t> m_pushConstants;                          // PushConstants(material, size, ptr)
    uint32_t m_casterDraws = 0;                                // depth-only draws recorded in the current pass (the first one clears)
    uint32_t m_surfaceDraws = 0;                               // Standard.shader draws recorded in the current pass (the first one begins the surface pass)
    bool m_bClearDepth = false;                                // BeginRenderPass(..., bClearDepthStencil): a surface pass then starts from cleared keys
    bool m_surfaceCutout = false;                              // ... one of them with ALPHA_CUTOUT: the pass ends with the depth write (sailor_hip_surface_store_depth)
    bool m_surfaceGltf = false;                                // ... one of them with Standard_glTF.shader: the pass ends with the glTF resolve and composite
    // the draws of materials WITHOUT z-write recorded in the current pass (the Transparent queue): nothing is launched per draw, the pass ends with the peel
    // over all of them.  m_bTransparentRefused: the pass mixed z-write on and off, or held an indirect transparent draw: it ends with the unsupported status
    struct TransparentDraw { TRefPtr<class RHIBuffer> m_vertexBuffer, m_indexBuffer; uint32_t m_indexCount, m_instanceCount, m_firstIndex, m_vertexOffset, m_firstInstance, m_flags; };
    TVector<TransparentDraw> m_transparentDraws;
    bool m_bTransparentRefused = false;
    TRefPtr<class RHIMaterial> m_boundMaterial;
    TVector<TRefPtr<class RHIShaderBindingSet>> m_boundBindings;
    bool m_bIndexUint16 = false;                               // BindIndexBuffer(..., bUint16InsteadOfUint32)
    ivec2 m_scissorOffset, m_scissorExtent;                    // SetViewport's scissor; an extent of (-1, -1): none set, the whole attachment
    // ImGuiUI.shader draws recorded in the current pass, each with the scissor that was set when it was recorded: the pass ends with ONE ordered blend over them
    TVector<SailorUiCommand> m_uiCommands;
    TVector<uint8_t> m_uiPushConstants;
    TRefPtr<class RHIBuffer> m_uiVertexBuffer, m_uiIndexBuffer;
    bool m_bUiIndexUint16 = false;
    TRefPtr<class RHITexture> m_uiTexture;                     // `sTexture` of the bound set
};
using RHICommandListPtr = TRefPtr<RHICommandList>;

} // namespace RHI
} // namespace Sailor
