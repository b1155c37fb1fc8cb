// Mirrors Runtime/FrameGraph/LightCullingNode.h:10-37.
#pragma once
#include "FrameGraphNode.h"
#include "SceneIndirectDraws.h"

namespace Sailor::Framegraph {

class LightCullingNode : public TFrameGraphNode<LightCullingNode> {
public:
    static const uint32_t LightsPerTile = 128; // LightCullingNode.h:15
    static const uint32_t TileSize = 16;       // LightCullingNode.h:16

    static const char* GetName() { return m_name; }

    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

    RHI::RHIShaderBindingSetPtr GetCulledLights() const { return m_culledLights; }

protected:
    using PushConstants = SailorLightCullPushConstants; // LightCullingNode.h:25-31 (88 bytes)

    static const char* m_name;
    RHI::RHIShaderPtr m_pComputeShader;
    RHI::RHIShaderBindingSetPtr m_culledLights;
};

// The pass in front of the cull: Runtime/FrameGraph/LinearizeDepthNode.h.  Resources: "depthStencil" = the raw reversed-Z
// depth attachment, "target" = the LinearDepth render target (DefaultRenderer.renderer: LinearizeDepth node).
class LinearizeDepthNode : public TFrameGraphNode<LinearizeDepthNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pLinearizeDepthShader;
    RHI::RHIMaterialPtr m_postEffectMaterial;
    RHI::RHIShaderBindingSetPtr m_linearizeDepth;
};

// The shading consumer of the lists: RenderSceneNode (FrameGraph/RenderSceneNode.cpp:109) records raster draws whose
// fragment shader is Standard.shader.  With a "surface" resource (3 float4 planes; "radiance" = float4 per pixel) the fragment work is one compute
// dispatch over that buffer, as before the surface pass existed.  Without one, and with batches in the scene view, the node records the reference's
// draws: BeginRenderPass("color", "depthStencil"), BindMaterial(Standard), BindShaderBindings, and per batch BindVertexBuffer / BindIndexBuffer /
// DrawIndexed, EndRenderPass -- the HIP backend rasterises, resolves, shades and composites behind them (sailor_hip_surface_*).
// The node's `Tag` is the render queue it draws (RenderSceneNode.cpp: `Tag: Opaque`, then `Tag: Masked` in DefaultRenderer.renderer): a batch is drawn if its own
// tag is empty or equal to the node's; a batch with ALPHA_CUTOUT is drawn with a material of CreateShader("Shaders/Standard.shader", { "ALPHA_CUTOUT" }).
// With the string `GPUCulling: true` those draws are DrawIndexedIndirect behind a "GPU Culling" dispatch on the transfer list (SceneIndirectDraws); "depthHighZ"
// switches the dispatch's OCCLUSION_CULLING on.
class RenderSceneNode : public TFrameGraphNode<RenderSceneNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pShader;
    RHI::RHIMaterialPtr m_pMaterial;
    // the materials of batches that are not the default one: [0] double-sided, [1] ALPHA_CUTOUT, [2] both (created when the first such batch is drawn)
    RHI::RHIShaderPtr m_pCutoutShader;
    RHI::RHIMaterialPtr m_pVariants[3];
    // the materials of glTF batches (RHISceneBatch::m_bGltf), Shaders/Standard_glTF.shader: [0] plain, [1] double-sided, [2] ALPHA_CUTOUT, [3] both
    RHI::RHIShaderPtr m_pGltfShader, m_pGltfCutoutShader;
    RHI::RHIMaterialPtr m_pGltfMaterials[4];
    // the materials of batches without z-write (the Transparent queue): [((gltf * 2 + ALPHA_CUTOUT) * 2 + double-sided) * 4 + blend mode]
    RHI::RHIMaterialPtr m_pTransparentMaterials[32];
    RHI::RHIShaderBindingSetPtr m_surfaceBindings;
    // `GPUCulling: true` (DefaultRenderer.renderer): the draws are recorded as RHIRecordDrawCallGPUCulling records them (SceneIndirectDraws.h); without the
    // string the node records DrawIndexed with host counts, as before
    SceneIndirectDraws m_draws;

public:
    const SceneIndirectDraws& GetIndirectDraws() const { return m_draws; }
};

// The one-off image-based-lighting bake: Runtime/FrameGraph/EnvironmentNode.h.  Raw environment = the frame graph's sampler
// "g_skyCubemap" (EnvironmentNode.cpp:139-142; the equirect-file branch needs the asset pipeline and is not mirrored); results are
// published as samplers "g_brdfSampler", "g_envCubemap", "g_irradianceCubemap" (:79, :187, :247), which RHIFrameGraph::Process binds
// into the lights set for Standard.shader's ambient term.
class EnvironmentNode : public TFrameGraphNode<EnvironmentNode> {
public:
    static constexpr uint32_t EnvMapSize = 512;       // EnvironmentNode.h:16 } the raw cube made from an equirect panorama; a sky cubemap
    static constexpr uint32_t EnvMapLevels = 10;      // EnvironmentNode.h:17 } published as g_skyCubemap brings its own size
    static constexpr uint32_t IrradianceMapSize = 32; // EnvironmentNode.h:19
    static constexpr uint32_t BrdfLutSize = 256;      // EnvironmentNode.h:20 (EnvMapSize / EnvMapLevels (:16-17) are taken from the raw cubemap here)
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;
    void MarkDirty() { m_bIsDirty = true; } // EnvironmentNode.h:28
    // EnvironmentNode.cpp:100-111 loads the "EnvironmentMap" asset through the TextureImporter (out of scope): the loaded texture is handed in
    void SetEnvironmentMap(RHI::RHITexturePtr equirect) { m_envMapTexture = equirect; m_envCubemap.Clear(); m_irradianceCubemap.Clear(); m_bIsDirty = true; }

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pComputeIrradianceShader, m_pComputeSpecularShader, m_pComputeBrdfShader;
    RHI::RHIShaderBindingSetPtr m_computeIrradianceBindings, m_computeSpecularBindings, m_computeBrdfBindings;
    RHI::RHICubemapPtr m_envCubemap, m_irradianceCubemap; // (keyed by the sky parameters in the reference: one sky here)
    RHI::RHITexturePtr m_brdfSampler;
    RHI::RHITexturePtr m_envMapTexture; // EnvironmentNode.h:43
    bool m_bIsDirty = false;
    // EnvironmentNode.cpp:150-175 keeps the baked cubes in maps keyed by the Sky node's parameters (SkyParams::operator==: the light direction times ten,
    // truncated).  One entry of that cache is kept here: a dirty mark under another key bakes again, under the same key it republishes the cubes.
    bool m_bHasSkyKey = false;
    int32_t m_skyKey[3] = { 0, 0, 0 };
};

// The Hi-Z pyramid builder: Runtime/FrameGraph/DepthHighZNode.h.  Resources: "src" = the (half-resolution) depth target, "dst" = the
// DepthHighZ render target with its mip chain (DefaultRenderer.renderer:51-57, :213-217).
class DepthHighZNode : public TFrameGraphNode<DepthHighZNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    struct PushConstantsDownscale { float m_outputSize[2]; }; // DepthHighZNode.h
    static const char* m_name;
    RHI::RHIShaderPtr m_pComputeDepthHighZShader;
    TVector<RHI::RHIShaderBindingSetPtr> m_computeDepthHighZBindings;
    RHI::RHIShaderBindingSetPtr m_computePrepassDepthHighZBindings;
};

// The first node behind the two RenderScene passes: Runtime/FrameGraph/EyeAdaptationNode.h.  Resources (DefaultRenderer.renderer:307-319): "hdrColor" = the
// HDR target the histogram is taken of, "colorSampler" = the HDR target the tone-mapping draw samples, "color" = the LDR target it writes.  Strings
// "toneMappingShader" / "toneMappingDefines", vec4 "data.whitePoint" / "data.exposure".
class EyeAdaptationNode : public TFrameGraphNode<EyeAdaptationNode> {
public:
    static const uint32_t HistogramShades = 256; // EyeAdaptationNode.h
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;
    RHI::RHITexturePtr GetAverageLuminance() const { return m_averageLuminance; }
    RHI::RHIShaderBindingSetPtr GetHistogramBindings() const { return m_computeHistogramShaderBindings; }

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pComputeHistogramShader, m_pComputeAverageShader, m_pToneMappingShader;
    RHI::RHIShaderBindingSetPtr m_computeHistogramShaderBindings, m_computeAverageShaderBindings, m_shaderBindings;
    RHI::RHIMaterialPtr m_postEffectMaterial;
    RHI::RHITexturePtr m_averageLuminance;
    float m_whitePointLum = 0.0f;
};

// The generic full-screen pass: Runtime/FrameGraph/PostProcessNode.h.  Strings "shader" / "defines", float and vec4 parameters named
// "<block>.<member>" (DefaultRenderer.renderer:222-230), resources: "color" = the target, every other name = a sampler of the shader.
class PostProcessNode : public TFrameGraphNode<PostProcessNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pShader;
    RHI::RHIMaterialPtr m_postEffectMaterial;
    RHI::RHIShaderBindingSetPtr m_shaderBindings;
};

// Runtime/FrameGraph/BlitNode.h without its MSAA half (BlitNode.cpp:90-122, BlitRaw): resources "src" and "dst".
class BlitNode : public TFrameGraphNode<BlitNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
};

// The atmosphere, the sun disk and g_skyCubemap: Runtime/FrameGraph/SkyNode.h.  Resources (DefaultRenderer.renderer:145-149): "color" = the Sky target,
// "linearDepth".  Drawn: Sky.shader {FILL}, {SUN}, {COMPOSE} every frame and {} into one face of g_skyCubemap per frame while dirty; with the cloud
// textures published (SetCloudTextures) and m_cloudsDensity > 0 also Sky.shader {CLOUDS} and the alpha-blended Blit.shader draw "Blit Clouds", otherwise
// the m_cloudsDensity == 0 branch (SkyNode.cpp:604-609).  For a driver that opted in (HipGraphicsDriver::EnableShader) also the star points in front of
// the clouds blit -- once the caller has published the star mesh (SetStars) -- and the sun-shaft draw behind it (SkyNode.cpp:692-747); without the opt-in
// Stars.shader and SunShafts.shader are created "not ready" and never recorded.  The node neither parses the catalogue (sailor_host_sky_star_mesh does),
// nor loads CloudsMap.png, nor generates the noise volumes.
class SkyNode : public TFrameGraphNode<SkyNode> {
public:
    static constexpr uint32_t EnvCubemapSize = 256u;      // SkyNode.h:13
    static constexpr uint32_t SkyResolution = 256u;       // SkyNode.h:14
    static constexpr uint32_t SunResolution = 32u;        // SkyNode.h:15
    static constexpr float CloudsResolutionFactor = 0.5f; // SkyNode.h:16
    using SkyParams = SailorSkyParams;                    // SkyNode.h:48-67 (member initialisers: sailor_host_sky_params_default)

    SkyNode() { sailor_host_sky_params_default(&m_skyParams); }
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

    RHI::RHIShaderBindingSetPtr GetShaderBindings() { return m_pShaderBindings; }
    void MarkDirty() { m_bIsDirty = true; m_updateEnvCubemapPattern = 0; } // SkyNode.h:103
    const SkyParams& GetSkyParams() const { return m_skyParams; }           // SkyNode.h:105
    SkyParams& GetSkyParams() { return m_skyParams; }                       // SkyNode.h:106
    uint32_t GetUpdateEnvCubemapPattern() const { return m_updateEnvCubemapPattern; } // (not in the reference: read-back for the tests)
    bool IsDirty() const { return m_bIsDirty; }
    // The clouds are opt-in (as the Bloom node is, FrameGraphNode.h): the reference loads Textures/CloudsMap.png and loads or generates the two noise
    // volumes itself (SkyNode.cpp:254-339); here the caller publishes the three textures, and until it has, the node records what it recorded without them
    void SetCloudTextures(RHI::RHITexturePtr map, RHI::RHITexturePtr noiseLow, RHI::RHITexturePtr noiseHigh)
    {
        m_pCloudsMapTexture = std::move(map); m_pCloudsNoiseLowTexture = std::move(noiseLow); m_pCloudsNoiseHighTexture = std::move(noiseHigh);
        m_bCloudTexturesChanged = true; // Process re-points bindings 3, 4 and 5 at them
    }
    bool HasCloudTextures() const { return m_pCloudsMapTexture && m_pCloudsNoiseLowTexture && m_pCloudsNoiseHighTexture; }
    // The star mesh (m_starsMesh, SkyNode.cpp:61-108), published by the caller like the cloud textures: until it has been, the star draw is left out and the
    // node otherwise works.  vertexBuffer: the VertexP3C4 mesh de-interleaved -- count x 3 floats of positions, then, at the next 16-byte boundary, count x 4
    // floats of colours (sailor_host_sky_star_mesh's two outputs); indexBuffer: count uint32, index i = i (:90)
    void SetStars(RHI::RHIBufferPtr vertexBuffer, RHI::RHIBufferPtr indexBuffer, uint32_t count)
    {
        m_starsVertexBuffer = std::move(vertexBuffer); m_starsIndexBuffer = std::move(indexBuffer); m_starsCount = count;
    }
    bool HasStars() const { return m_starsVertexBuffer && m_starsIndexBuffer; }

protected:
    static const char* m_name;
    SkyParams m_skyParams {};
    RHI::RHIShaderPtr m_pSunShader, m_pSkyShader, m_pSkyEnvShader, m_pStarsShader, m_pComposeShader, m_pCloudsShader, m_pSunShaftsShader, m_pBlitShader;
    RHI::RHIMaterialPtr m_pStarsMaterial, m_pSkyMaterial, m_pSkyEnvMaterial, m_pSunMaterial, m_pComposeMaterial, m_pCloudsMaterial, m_pSunShaftsMaterial,
        m_pBlitCloudsMaterial;
    RHI::RHIShaderBindingSetPtr m_pShaderBindings, m_pBlitCloudsBindings, m_pEnvCubemapBindings[6];
    RHI::RHITexturePtr m_pSkyTexture, m_pSunTexture, m_pCloudsTexture, m_pCloudsMapTexture, m_pCloudsNoiseLowTexture, m_pCloudsNoiseHighTexture;
    RHI::RHIBufferPtr m_starsVertexBuffer, m_starsIndexBuffer; // m_starsMesh (SkyNode.h:151)
    uint32_t m_starsCount = 0;
    uint32_t m_ditherPatternIndex = 0;
    uint32_t m_updateEnvCubemapPattern = 0; // SkyNode.h:173
    bool m_bIsDirty = true;                 // SkyNode.h:174
    bool m_bCloudTexturesChanged = false;
};

// Everything DebugContext collected, behind the RenderScene passes: Runtime/FrameGraph/DebugDrawNode.{h,cpp}.  Resources (DefaultRenderer.renderer:289-293):
// "color" = Main, "depthStencil" = DepthBuffer (the default when none is given, DebugDrawNode.cpp:30-34).  The reference replays a SECONDARY command list the
// world recorded DebugContext::DrawDebugMesh(projection * view) into (RenderSecondaryCommandBuffers, :51-76); this mirror has no secondary lists, so the node
// records the same calls DIRECTLY into its command list: BeginRenderPass(color, depthStencil), DrawDebugMesh of the scene view's context, EndRenderPass.
class DebugDrawNode : public TFrameGraphNode<DebugDrawNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
};

// The editor's UI over the finished frame: Runtime/FrameGraph/RenderImGuiNode.{h,cpp}.  Resources (DefaultRenderer.renderer, the last entry): "color" =
// BackBuffer, "depthStencil" = DepthBuffer.  The reference waits for the task that recorded ImGuiApi::ImGui_RenderDrawData (Submodules/ImGuiApi.cpp:190-276)
// into a SECONDARY command list and replays it (RenderSecondaryCommandBuffers, no clear, :21-60); this mirror has no secondary lists, so the node records the
// same calls DIRECTLY into its command list from the snapshot's draw data: BindMaterial, BindVertexBuffer, BindIndexBuffer (16-bit), SetViewport,
// PushConstants, and per command SetViewport with its scissor, BindShaderBindings and DrawIndexed.
class RenderImGuiNode : public TFrameGraphNode<RenderImGuiNode> {
public:
    static const char* GetName() { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
};

// The mip pyramid over `Main`: Runtime/FrameGraph/BloomNode.h.  Resource (DefaultRenderer.renderer:303-304): "bloom" = the HDR target with its mip chain,
// rewritten in place; vec4 "threshold", "knee", "bloomIntensity", "dirtIntensity" (their .x).  `u_dirt_texture` is the graph's "g_lensDirtSampler".
// In the reference this is a TFrameGraphNode<BloomNode> (BloomNode.h:10, :43) and registers under "Bloom"; here the class derives from the base directly
// and is created by FrameGraphBuilder::CreateOptInNode for graphs that enabled it (FrameGraphNode.h says why).
class BloomNode : public BaseFrameGraphNode {
public:
    static const char* GetName() { return m_name; }
    std::string GetDebugName() const override { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

protected:
    static const char* m_name;
    RHI::RHIShaderPtr m_pComputeDownscaleShader, m_pComputeUpscaleShader;
    TVector<RHI::RHIShaderBindingSetPtr> m_computeDownscaleBindings, m_computeUpscaleBindings;
    struct PushConstantsDownscale { // BloomNode.h:28-32
        float m_threshold[4];       // x -> threshold, yzw -> (threshold - knee, 2.0 * knee, 0.25 * knee)
        bool m_useThreshold;
    };
    struct PushConstantsUpscale { // BloomNode.h:34-39
        uint32_t m_mipLevel;
        float m_bloomIntensity;
        float m_dirtIntensity;
    };
};

} // namespace Sailor::Framegraph
