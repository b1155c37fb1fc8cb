#include <algorithm>
#include <cmath>
#include <sstream>
#include "FrameGraphNode.h"
#include "LightCullingNode.h"
#include "DepthPrepassNode.h"
#include "ShadowPrepassNode.h"
#include "ClearNode.h"
#include "ParticlesNode.h"
#include "RHIFrameGraph.h"
#include "../RHI/Renderer.h"
#include "../RHI/DebugContext.h"

using namespace Sailor;
using namespace Sailor::RHI;
using namespace Sailor::Framegraph;

// ---- FrameGraphBuilder (FrameGraph/FrameGraphNode.cpp:16-41) -----------------------------------------------------------------
std::map<std::string, std::function<FrameGraphNodePtr(void)>>& FrameGraphBuilder::Registry()
{
    static std::map<std::string, std::function<FrameGraphNodePtr(void)>> s_nodes; // function-local: safe during static init
    return s_nodes;
}

void FrameGraphBuilder::RegisterFrameGraphNode(const std::string& nodeName, std::function<FrameGraphNodePtr(void)> factoryMethod)
{
    Registry()[nodeName] = std::move(factoryMethod);
}

FrameGraphNodePtr FrameGraphBuilder::CreateNode(const std::string& nodeName)
{
    auto it = Registry().find(nodeName);
    return it == Registry().end() ? FrameGraphNodePtr() : it->second();
}

bool FrameGraphBuilder::IsRegistered(const std::string& nodeName) { return Registry().count(nodeName) != 0; }

FrameGraphNodePtr FrameGraphBuilder::CreateOptInNode(const std::string& nodeName)
{
    if (nodeName == BloomNode::GetName()) return FrameGraphNodePtr(new BloomNode());
    if (nodeName == ShadowPrepassNode::GetName()) return FrameGraphNodePtr(new ShadowPrepassNode());
    if (nodeName == ClearNode::GetName()) return FrameGraphNodePtr(new ClearNode());
    if (nodeName == ParticlesNode::GetName()) return FrameGraphNodePtr(new ParticlesNode());
    return FrameGraphNodePtr();
}

// force the registration objects of the path's nodes into the library
template class Sailor::Framegraph::TFrameGraphNode<LightCullingNode>;
template class Sailor::Framegraph::TFrameGraphNode<RenderSceneNode>;
template class Sailor::Framegraph::TFrameGraphNode<DepthPrepassNode>;
template class Sailor::Framegraph::TFrameGraphNode<LinearizeDepthNode>;
template class Sailor::Framegraph::TFrameGraphNode<EnvironmentNode>;
template class Sailor::Framegraph::TFrameGraphNode<DepthHighZNode>;
template class Sailor::Framegraph::TFrameGraphNode<EyeAdaptationNode>;
template class Sailor::Framegraph::TFrameGraphNode<PostProcessNode>;
template class Sailor::Framegraph::TFrameGraphNode<BlitNode>;
template class Sailor::Framegraph::TFrameGraphNode<SkyNode>;
template class Sailor::Framegraph::TFrameGraphNode<DebugDrawNode>;
template class Sailor::Framegraph::TFrameGraphNode<RenderImGuiNode>;

// ---- RHIFrameGraph ----------------------------------------------------------------------------------------------------------
UboFrameData RHIFrameGraph::FillFrameData(RHICommandListPtr transferCmdList, RHISceneViewSnapshot& snapshot, const UboFrameData& previousFrame, float deltaTime,
                                          float worldTime) const
{
    // RHIFrameGraph.cpp:56-70
    UboFrameData frameData {};
    snapshot.m_frameBindings = Renderer::GetDriver()->CreateShaderBindings();
    Renderer::GetDriver()->AddBufferToShaderBindings(snapshot.m_frameBindings, "frameData", sizeof(UboFrameData), 0, EShaderBindingType::UniformBuffer);
    Renderer::GetDriver()->AddBufferToShaderBindings(snapshot.m_frameBindings, "previousFrameData", sizeof(UboFrameData), 1, EShaderBindingType::UniformBuffer); // (:58)
    sailor_host_fill_frame_data(snapshot.m_camera.m_world, snapshot.m_camera.m_fov, snapshot.m_camera.m_aspect, snapshot.m_camera.m_zNear,
                                snapshot.m_camera.m_zFar, m_viewport.x, m_viewport.y, worldTime, deltaTime, &frameData);
    Renderer::GetDriverCommands()->UpdateShaderBinding(transferCmdList, snapshot.m_frameBindings->GetOrAddShaderBinding("frameData"), &frameData, sizeof(frameData));
    Renderer::GetDriverCommands()->UpdateShaderBinding(transferCmdList, snapshot.m_frameBindings->GetOrAddShaderBinding("previousFrameData"), &previousFrame,
                                                       sizeof(previousFrame)); // (:70)
    return frameData;
}

void RHIFrameGraph::Process(RHISceneViewSnapshot& snapshot)
{
    auto driver = Renderer::GetDriver();
    auto transferCmdList = driver->CreateCommandList();
    auto cmdList = driver->CreateCommandList();
    const FrameCaptureHook capture = std::move(m_captureHook); // armed for this frame alone (RHIFrameGraph.h)
    m_captureHook = nullptr;
    if (capture) capture(transferCmdList, CaptureSlotFrameStart);
    m_prevFrameData = FillFrameData(transferCmdList, snapshot, m_prevFrameData, snapshot.m_deltaTime, snapshot.m_currentTime); // (:189)
    if (snapshot.m_rhiLightsData) { // RHIFrameGraph.cpp:128-163: the IBL samplers and the AO target join the lights set (bindings 3, 4, 5, 9)
        struct { const char* name; RHITexturePtr tex; uint32_t binding; } ibl[] = {
            { "g_irradianceCubemap", GetSampler("g_irradianceCubemap"), 3 }, { "g_brdfSampler", GetSampler("g_brdfSampler"), 4 },
            { "g_envCubemap", GetSampler("g_envCubemap"), 5 }, { "g_aoSampler", GetRenderTarget("g_AO"), 9 } };
        for (auto& e : ibl) {
            if (!e.tex) continue;
            auto b = snapshot.m_rhiLightsData->Find(e.name);
            if (!b || b->m_textures.empty() || b->m_textures[0].GetRawPtr() != e.tex.GetRawPtr())
                driver->AddSamplerToShaderBindings(snapshot.m_rhiLightsData, e.name, e.tex, e.binding);
        }
    }
    for (auto& node : m_graph) node->Prepare(this, snapshot);
    if (capture) capture(cmdList, CaptureSlotBeforeNodes);
    int slot = CaptureSlotFirstNode;
    for (auto& node : m_graph) {
        node->Process(this, transferCmdList, cmdList, snapshot); // RHIFrameGraph.cpp:250-252
        if (capture) capture(cmdList, slot++);
    }
    driver->SubmitCommandList(transferCmdList);
    driver->SubmitCommandList(cmdList);
}

void RHIFrameGraph::Clear()
{
    for (auto& node : m_graph) node->Clear();
    m_graph.clear();
    m_renderTargets.clear();
    m_prevFrameData = UboFrameData {}; // (a graph built next starts with a first frame)
    m_captureHook = nullptr;
}

// ---- EnvironmentNode (FrameGraph/EnvironmentNode.cpp:19-281) --------------------------------------------------------------------
const char* EnvironmentNode::m_name = "Environment";

void EnvironmentNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot&)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName());
    if (!m_pComputeBrdfShader) { m_pComputeBrdfShader = driver->CreateShader("Shaders/ComputeBrdfLut.shader"); m_computeBrdfBindings = driver->CreateShaderBindings(); }                 // (:31-39)
    if (!m_pComputeSpecularShader) { m_pComputeSpecularShader = driver->CreateShader("Shaders/ComputeEnvMap_IBL.shader"); m_computeSpecularBindings = driver->CreateShaderBindings(); } // (:41-49)
    if (!m_pComputeIrradianceShader) { m_pComputeIrradianceShader = driver->CreateShader("Shaders/ComputeIrradianceMap.shader"); m_computeIrradianceBindings = driver->CreateShaderBindings(); } // (:51-59)

    if (!m_brdfSampler) { // (:69-98)
        m_brdfSampler = driver->CreateRenderTarget({ (int32_t)BrdfLutSize, (int32_t)BrdfLutSize }, 1, EFormat::R32G32_SFLOAT);
        commands->ImageMemoryBarrier(commandList, m_brdfSampler, EImageLayout::ShaderReadOnlyOptimal);
        frameGraph->SetSampler("g_brdfSampler", m_brdfSampler);
        commands->BeginDebugRegion(commandList, "Generate Cook-Torrance BRDF 2D LUT for split-sum approximation");
        driver->AddStorageImageToShaderBindings(m_computeBrdfBindings, "dst", m_brdfSampler, 0);
        commands->ImageMemoryBarrier(commandList, m_brdfSampler, EImageLayout::ComputeWrite);
        commands->Dispatch(commandList, m_pComputeBrdfShader, (uint32_t)(m_brdfSampler->GetExtent().x / 32.0f), (uint32_t)(m_brdfSampler->GetExtent().y / 32.0f), 6u,
                           { m_computeBrdfBindings }, nullptr, 0);
        commands->ImageMemoryBarrier(commandList, m_brdfSampler, EImageLayout::ShaderReadOnlyOptimal);
        commands->EndDebugRegion(commandList);
    }

    if (m_bIsDirty) { // (:100-276)
        RHICubemapPtr rawEnvCubemap;
        if (m_envMapTexture) { // (:116-138) the panorama -> the raw cube and its mip chain
            rawEnvCubemap = driver->CreateCubemap({ (int32_t)EnvMapSize, (int32_t)EnvMapSize }, EnvMapLevels, EFormat::R32G32B32A32_SFLOAT);
            commands->ImageMemoryBarrier(commandList, rawEnvCubemap, EImageLayout::ShaderReadOnlyOptimal);
            commands->BeginDebugRegion(commandList, "Generate Raw Env Cubemap from Equirect");
            commands->ImageMemoryBarrier(commandList, rawEnvCubemap, EImageLayout::ComputeWrite);
            commands->ConvertEquirect2Cubemap(commandList, m_envMapTexture, rawEnvCubemap);
            commands->ImageMemoryBarrier(commandList, rawEnvCubemap, EImageLayout::TransferDstOptimal);
            commands->GenerateMipMaps(commandList, rawEnvCubemap);
            commands->EndDebugRegion(commandList);
            frameGraph->SetSampler("g_rawEnvCubemap", rawEnvCubemap); // not in the reference: lets the harness read the intermediate back
        } else {
            rawEnvCubemap = frameGraph->GetSampler("g_skyCubemap"); // (:139-142)
        }
        if (!rawEnvCubemap || !rawEnvCubemap->m_bCubemap) { commands->EndDebugRegion(commandList); return; } // (:143-146)
        const int32_t EnvMapSize = rawEnvCubemap->GetExtent().x;
        const uint32_t EnvMapLevels = rawEnvCubemap->GetMipLevels();
        if (!m_envMapTexture) // (:150-162) the cubes belong to the Sky node's parameters
            if (auto pSkyNode = frameGraph->GetGraphNode("Sky").DynamicCast<SkyNode>()) {
                int32_t key[3];
                for (int k = 0; k < 3; k++) key[k] = (int32_t)(pSkyNode->GetSkyParams().lightDirection[k] * 10.0f); // SkyNode.h:85-88
                if (m_bHasSkyKey && (key[0] != m_skyKey[0] || key[1] != m_skyKey[1] || key[2] != m_skyKey[2])) { m_envCubemap.Clear(); m_irradianceCubemap.Clear(); }
                for (int k = 0; k < 3; k++) m_skyKey[k] = key[k];
                m_bHasSkyKey = true;
            }
        const bool bShouldUpdateEnvCubemap = !m_envCubemap, bShouldUpdateIrradianceCubemap = !m_irradianceCubemap; // (:162-163)
        if (!bShouldUpdateEnvCubemap && !bShouldUpdateIrradianceCubemap) { // (:165-173)
            frameGraph->SetSampler("g_envCubemap", m_envCubemap);
            frameGraph->SetSampler("g_irradianceCubemap", m_irradianceCubemap);
            m_bIsDirty = false;
            commands->EndDebugRegion(commandList);
            return;
        }
        if (bShouldUpdateEnvCubemap) { // (:176-236)
            m_envCubemap = driver->CreateCubemap({ EnvMapSize, EnvMapSize }, EnvMapLevels, EFormat::R32G32B32A32_SFLOAT);
            frameGraph->SetSampler("g_envCubemap", m_envCubemap);
            commands->ImageMemoryBarrier(commandList, m_envCubemap, EImageLayout::General);
            commands->BeginDebugRegion(commandList, "Compute pre-filtered specular environment map");
            struct PushConstants { int32_t level {}; float roughness {}; };
            const uint32_t NumMipTailLevels = EnvMapLevels - 1;
            commands->ImageMemoryBarrier(commandList, rawEnvCubemap, EImageLayout::TransferSrcOptimal);
            commands->ImageMemoryBarrier(commandList, m_envCubemap, EImageLayout::TransferDstOptimal);
            commands->BlitImage(commandList, rawEnvCubemap, m_envCubemap, { 0, 0, EnvMapSize, EnvMapSize }, { 0, 0, EnvMapSize, EnvMapSize }); // (:200-203) mip 0
            commands->ImageMemoryBarrier(commandList, rawEnvCubemap, EImageLayout::ShaderReadOnlyOptimal);
            commands->ImageMemoryBarrier(commandList, m_envCubemap, EImageLayout::ComputeWrite);
            TVector<RHITexturePtr> envMapMips; // the mip tail (:208-212)
            for (uint32_t level = 1; level < EnvMapLevels; ++level) envMapMips.push_back(m_envCubemap->GetMipLevel(level));
            driver->AddSamplerToShaderBindings(m_computeSpecularBindings, "rawEnvMap", rawEnvCubemap, 0);
            driver->AddStorageImageToShaderBindings(m_computeSpecularBindings, "envMap", envMapMips, 1);
            const float deltaRoughness = 1.0f / std::max(float(NumMipTailLevels), 1.0f);
            for (uint32_t level = 1, size = (uint32_t)EnvMapSize / 2; level < EnvMapLevels; ++level, size /= 2) { // (:220-233)
                const uint32_t numGroups = std::max<uint32_t>(1u, size / 32u);
                const PushConstants pushConstants = { (int32_t)(level - 1u), level * deltaRoughness };
                commands->Dispatch(commandList, m_pComputeSpecularShader, numGroups, numGroups, 6u, { m_computeSpecularBindings }, &pushConstants, sizeof(PushConstants));
            }
            commands->EndDebugRegion(commandList);
        }
        if (bShouldUpdateIrradianceCubemap) { // (:238-273)
            int32_t irradianceSize = (int32_t)IrradianceMapSize;
            float overrideSize = 0.0f;
            if (TryGetFloat("IrradianceMapSize", overrideSize) && overrideSize >= 1.0f) irradianceSize = (int32_t)overrideSize; // test knob (65 536 samples per texel)
            m_irradianceCubemap = driver->CreateCubemap({ irradianceSize, irradianceSize }, 1, EFormat::R32G32B32A32_SFLOAT);
            commands->ImageMemoryBarrier(commandList, m_irradianceCubemap, EImageLayout::ShaderReadOnlyOptimal);
            frameGraph->SetSampler("g_irradianceCubemap", m_irradianceCubemap);
            commands->ImageMemoryBarrier(commandList, m_irradianceCubemap, EImageLayout::General);
            commands->BeginDebugRegion(commandList, "Compute diffuse irradiance cubemap");
            commands->ImageMemoryBarrier(commandList, m_envCubemap, EImageLayout::ShaderReadOnlyOptimal);
            commands->ImageMemoryBarrier(commandList, m_irradianceCubemap, EImageLayout::ComputeWrite);
            driver->AddSamplerToShaderBindings(m_computeIrradianceBindings, "envMap", m_envCubemap, 0);
            driver->AddStorageImageToShaderBindings(m_computeIrradianceBindings, "irradianceMap", m_irradianceCubemap, 1);
            commands->Dispatch(commandList, m_pComputeIrradianceShader, std::max(1u, (uint32_t)irradianceSize / 32u), std::max(1u, (uint32_t)irradianceSize / 32u), 6u,
                               { m_computeIrradianceBindings });
            commands->EndDebugRegion(commandList);
        }
        m_bIsDirty = false;
    }
    commands->EndDebugRegion(commandList);
}

void EnvironmentNode::Clear()
{
    m_pComputeIrradianceShader.Clear(); m_pComputeSpecularShader.Clear(); m_pComputeBrdfShader.Clear();
    m_computeIrradianceBindings.Clear(); m_computeSpecularBindings.Clear(); m_computeBrdfBindings.Clear();
    m_envCubemap.Clear(); m_irradianceCubemap.Clear(); m_brdfSampler.Clear(); m_envMapTexture.Clear();
}

// ---- DepthHighZNode (FrameGraph/DepthHighZNode.cpp:17-103) -----------------------------------------------------------------------
const char* DepthHighZNode::m_name = "DepthHighZ";

void DepthHighZNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot&)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto depthAttachment = GetRHIResource("src").DynamicCast<RHITexture>(); // (:28-32)
    if (!depthAttachment) depthAttachment = frameGraph->GetRenderTarget("DepthBuffer");
    auto highZRenderTarget = GetRHIResource("dst").DynamicCast<RHITexture>(); // (:34)
    if (!depthAttachment || !highZRenderTarget) return;
    if (!m_pComputeDepthHighZShader) m_pComputeDepthHighZShader = driver->CreateShader("Shaders/ComputeDepthHighZ.shader"); // (:38-44)
    if (m_computeDepthHighZBindings.empty()) { // (:51-67)
        m_computeDepthHighZBindings.resize(highZRenderTarget->GetMipLevels() - 1);
        for (uint32_t i = 0; i < highZRenderTarget->GetMipLevels() - 1; ++i) {
            auto readMipLevel = highZRenderTarget->GetMipLevel(i), writeMipLevel = highZRenderTarget->GetMipLevel(i + 1); // GetMipLayer
            m_computeDepthHighZBindings[i] = driver->CreateShaderBindings();
            driver->AddSamplerToShaderBindings(m_computeDepthHighZBindings[i], "inputDepth", readMipLevel, 0);
            driver->AddStorageImageToShaderBindings(m_computeDepthHighZBindings[i], "outputDepth", writeMipLevel, 1);
        }
        m_computePrepassDepthHighZBindings = driver->CreateShaderBindings();
        driver->AddSamplerToShaderBindings(m_computePrepassDepthHighZBindings, "inputDepth", depthAttachment, 0);
        driver->AddStorageImageToShaderBindings(m_computePrepassDepthHighZBindings, "outputDepth", highZRenderTarget->GetMipLevel(0), 1);
    }
    commands->BeginDebugRegion(commandList, GetName());
    commands->ImageMemoryBarrier(commandList, highZRenderTarget, EImageLayout::General);
    for (int32_t i = -1; i < (int32_t)highZRenderTarget->GetMipLevels() - 1; ++i) { // Depth Downscale (:78-96)
        const bool bFirst = i == -1;
        auto readMipLevel = bFirst ? depthAttachment : highZRenderTarget->GetMipLevel((uint32_t)i);
        auto writeMipLevel = highZRenderTarget->GetMipLevel((uint32_t)(i + 1));
        PushConstantsDownscale params {};
        params.m_outputSize[0] = (float)writeMipLevel->GetExtent().x; params.m_outputSize[1] = (float)writeMipLevel->GetExtent().y;
        commands->ImageMemoryBarrier(commandList, readMipLevel, EImageLayout::ShaderReadOnlyOptimal);
        commands->ImageMemoryBarrier(commandList, writeMipLevel, EImageLayout::ComputeWrite);
        commands->Dispatch(commandList, m_pComputeDepthHighZShader, (uint32_t)std::ceil(params.m_outputSize[0] / 8), (uint32_t)std::ceil(params.m_outputSize[1] / 8), 1u,
                           { bFirst ? m_computePrepassDepthHighZBindings : m_computeDepthHighZBindings[(size_t)i] }, &params, sizeof(PushConstantsDownscale));
    }
    commands->EndDebugRegion(commandList);
}

void DepthHighZNode::Clear()
{
    m_pComputeDepthHighZShader.Clear();
    m_computeDepthHighZBindings.clear();
    m_computePrepassDepthHighZBindings.Clear();
}

// ---- LinearizeDepthNode (FrameGraph/LinearizeDepthNode.cpp:18-109) -------------------------------------------------------------
const char* LinearizeDepthNode::m_name = "LinearizeDepth";

void LinearizeDepthNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName());

    auto depthAttachment = GetRHIResource("depthStencil").DynamicCast<RHITexture>(); // (:29-37)
    for (const auto& r : m_unresolvedResourceParams)
        if (r.first == "depthStencil") { depthAttachment = frameGraph->GetRenderTarget(r.second); break; }
    if (!depthAttachment) depthAttachment = frameGraph->GetRenderTarget("DepthBuffer");
    if (!m_pLinearizeDepthShader) m_pLinearizeDepthShader = driver->CreateShader("Shaders/LinearizeDepth.shader"); // (:39-43)
    auto target = GetRHIResource("target").DynamicCast<RHITexture>();                                                // (:45)
    if (!m_pLinearizeDepthShader || !target || !depthAttachment) { // (:47-50) silent early return
        commands->EndDebugRegion(commandList);
        return;
    }
    if (!m_linearizeDepth) { // (:52-56)
        m_linearizeDepth = driver->CreateShaderBindings();
        driver->AddSamplerToShaderBindings(m_linearizeDepth, "depthSampler", depthAttachment, 0);
    }
    if (!m_postEffectMaterial) m_postEffectMaterial = driver->CreateMaterial(m_pLinearizeDepthShader); // (:58-63)

    commands->ImageMemoryBarrier(commandList, depthAttachment, EImageLayout::ShaderReadOnlyOptimal); // (:79)
    commands->ImageMemoryBarrier(commandList, target, EImageLayout::ColorAttachmentOptimal);          // (:80)
    commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { target }, RHITexturePtr());       // (:84-92)
    commands->BindMaterial(commandList, m_postEffectMaterial);                                         // (:94)
    commands->BindShaderBindings(commandList, m_postEffectMaterial, { sceneView.m_frameBindings, m_linearizeDepth }); // (:98)
    commands->DrawIndexed(commandList, 6, 1, 0, 0, 0);                                                 // (:105) the full-screen NDC quad
    commands->EndRenderPass(commandList);                                                              // (:106)
    commands->EndDebugRegion(commandList);
}

void LinearizeDepthNode::Clear()
{
    m_linearizeDepth.Clear();
    m_postEffectMaterial.Clear();
    m_pLinearizeDepthShader.Clear();
}

// ---- LightCullingNode (FrameGraph/LightCullingNode.cpp:17-87) ------------------------------------------------------------------
const char* LightCullingNode::m_name = "LightCulling";

void LightCullingNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    if (!sceneView.m_rhiLightsData) return; // no point to cull lights if we have no lights in the scene (:24-28)

    auto driver = Renderer::GetDriver();
    if (!m_pComputeShader) m_pComputeShader = driver->CreateShader("Shaders/ComputeLightCulling.shader"); // (:30-34)

    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName());

    auto depthAttachment = GetRHIResource("depthStencil").DynamicCast<RHITexture>(); // DefaultRenderer.renderer:127-130 -> LinearDepth
    if (!depthAttachment) depthAttachment = frameGraph->GetRenderTarget("DepthBuffer");
    if (depthAttachment) {
        PushConstants pushConstants {};
        pushConstants.lightsNum = (int32_t)sceneView.m_totalNumLights;
        pushConstants.viewportSize[0] = depthAttachment->GetExtent().x;
        pushConstants.viewportSize[1] = depthAttachment->GetExtent().y;
        pushConstants.numTiles[0] = (depthAttachment->GetExtent().x - 1) / (int32_t)TileSize + 1; // (:56)
        pushConstants.numTiles[1] = (depthAttachment->GetExtent().y - 1) / (int32_t)TileSize + 1; // (:57)

        if (!m_culledLights) {
            const size_t numTiles = (size_t)pushConstants.numTiles[0] * pushConstants.numTiles[1];
            m_culledLights = driver->CreateShaderBindings();
            // +1: the reference's buffer is one uint short when every tile is full (:64)
            auto culledLightsSSBO = driver->AddSsboToShaderBindings(m_culledLights, "culledLights", sizeof(uint32_t) * (numTiles * LightsPerTile + 1), 1, 0, true);
            auto lightsGridSSBO = driver->AddSsboToShaderBindings(m_culledLights, "lightsGrid", sizeof(uint32_t) * (numTiles * 2 + 1), 1, 1, true);
            driver->AddSamplerToShaderBindings(m_culledLights, "sceneDepth", depthAttachment, 2);
            auto shaderBindingSet = sceneView.m_rhiLightsData;
            driver->AddShaderBinding(shaderBindingSet, culledLightsSSBO, "culledLights", 1); // (:69) so that Standard.shader sees them
            driver->AddShaderBinding(shaderBindingSet, lightsGridSSBO, "lightsGrid", 2);      // (:70)
        }

        commands->ImageMemoryBarrier(commandList, depthAttachment, EImageLayout::ShaderReadOnlyOptimal);
        commands->Dispatch(commandList, m_pComputeShader, (uint32_t)pushConstants.numTiles[0], (uint32_t)pushConstants.numTiles[1], 1,
                           { sceneView.m_rhiLightsData, m_culledLights, sceneView.m_frameBindings }, &pushConstants, sizeof(PushConstants));
    }
    commands->EndDebugRegion(commandList);
}

void LightCullingNode::Clear()
{
    m_pComputeShader.Clear();
    m_culledLights.Clear();
}

// ---- RenderSceneNode (shading consumer) ---------------------------------------------------------------------------------------
const char* RenderSceneNode::m_name = "RenderScene";

void RenderSceneNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr transferCommandList, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    if (!sceneView.m_rhiLightsData || !sceneView.m_rhiLightsData->Find("culledLights")) return; // RenderSceneNode.cpp:142-146: silent early return
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    if (!m_pShader) m_pShader = driver->CreateShader("Shaders/Standard.shader");
    auto surface = GetRHIResource("surface").DynamicCast<RHIBuffer>();
    auto radiance = GetRHIResource("radiance").DynamicCast<RHIBuffer>();
    if (!surface && !sceneView.m_batches.empty()) { // the reference's own recording (RenderSceneNode.cpp): real draws into (color, depthStencil)
        auto resolved = [&](const char* name) -> RHITexturePtr { // GetRHIResource / GetResolvedAttachment: a per-frame target is looked up by its name
            if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
            auto it = m_unresolvedResourceParams.find(name);
            return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
        };
        auto color = resolved("color");
        auto depth = resolved("depthStencil");
        if (!color) return;
        if (!m_pMaterial) m_pMaterial = driver->CreateMaterial(m_pShader);
        std::string tag;
        const bool tagged = TryGetString("Tag", tag);
        // `GPUCulling: true`: the Batch.hpp:53-191 sequence -- the node's own records and commands, the cull on the transfer list, indirect draws
        std::string culling;
        const bool gpuCulling = TryGetString("GPUCulling", culling) && culling == "true";
        RHIShaderBindingSetPtr sceneSet = sceneView.m_sceneBindings;
        if (gpuCulling) {
            TVector<size_t> selected;
            for (size_t i = 0; i < sceneView.m_batches.size(); i++)
                if (sceneView.m_batches[i].m_tag.empty() || (tagged && sceneView.m_batches[i].m_tag == tag)) selected.push_back(i);
            sceneSet = m_draws.Update(transferCommandList, sceneView, selected, true, resolved("depthHighZ"));
            if (!sceneSet) return; // nothing of this queue in the view
        }
        commands->BeginDebugRegion(commandList, std::string(GetName()) + (tagged ? " QueueTag:" + tag : ""));
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { color }, depth);
        commands->BindMaterial(commandList, m_pMaterial);
        commands->BindShaderBindings(commandList, m_pMaterial, { sceneView.m_frameBindings, sceneView.m_rhiLightsData, sceneSet });
        RHIMaterialPtr bound = m_pMaterial;
        size_t command = 0;
        for (const auto& b : sceneView.m_batches) {
            if (!b.m_tag.empty() && !(tagged && b.m_tag == tag)) continue; // the render queue filter: an untagged batch belongs to every queue
            RHIMaterialPtr material = m_pMaterial;
            if (!b.m_bZWrite) { // a material of the Transparent queue (ModelImporter.cpp:213-229): depth test, no depth write, the batch's blend mode
                RHIMaterialPtr& variant = m_pTransparentMaterials[(((b.m_bGltf ? 2 : 0) + (b.m_bAlphaCutout ? 1 : 0)) * 2 + (b.m_bDoubleSided ? 1 : 0)) * 4 + (int)b.m_blendMode];
                if (!variant) {
                    const char* path = b.m_bGltf ? "Shaders/Standard_glTF.shader" : "Shaders/Standard.shader";
                    variant = driver->CreateMaterial(b.m_bAlphaCutout ? driver->CreateShader(path, { "ALPHA_CUTOUT" }) : driver->CreateShader(path));
                    variant->m_bDoubleSided = b.m_bDoubleSided;
                    variant->m_bZWrite = false;
                    variant->m_blendMode = b.m_blendMode;
                }
                material = variant;
            } else if (b.m_bGltf) { // an imported model's material: Standard_glTF.shader (ModelImporter.cpp:156-231), with the same two variations
                RHIMaterialPtr& variant = m_pGltfMaterials[(b.m_bAlphaCutout ? 2 : 0) + (b.m_bDoubleSided ? 1 : 0)];
                if (!variant) {
                    RHIShaderPtr& shader = b.m_bAlphaCutout ? m_pGltfCutoutShader : m_pGltfShader;
                    if (!shader) shader = b.m_bAlphaCutout ? driver->CreateShader("Shaders/Standard_glTF.shader", { "ALPHA_CUTOUT" }) : driver->CreateShader("Shaders/Standard_glTF.shader");
                    variant = driver->CreateMaterial(shader);
                    variant->m_bDoubleSided = b.m_bDoubleSided;
                }
                material = variant;
            } else if (b.m_bAlphaCutout || b.m_bDoubleSided) { // the batch's own material: the ALPHA_CUTOUT permutation (ModelImporter.cpp:213-229), ECullMode::None
                RHIMaterialPtr& variant = m_pVariants[(b.m_bAlphaCutout ? 2 : 0) + (b.m_bDoubleSided ? 1 : 0) - 1];
                if (!variant) {
                    if (b.m_bAlphaCutout && !m_pCutoutShader) m_pCutoutShader = driver->CreateShader("Shaders/Standard.shader", { "ALPHA_CUTOUT" });
                    variant = driver->CreateMaterial(b.m_bAlphaCutout ? m_pCutoutShader : m_pShader);
                    variant->m_bDoubleSided = b.m_bDoubleSided;
                }
                material = variant;
            }
            if (material.GetRawPtr() != bound.GetRawPtr()) { commands->BindMaterial(commandList, material); bound = material; }
            if (gpuCulling) { m_draws.Draw(commandList, b, command++); continue; }
            commands->BindVertexBuffer(commandList, b.m_vertexBuffer, 0);
            commands->BindIndexBuffer(commandList, b.m_indexBuffer, 0);
            commands->DrawIndexed(commandList, b.m_indexCount, b.m_instanceCount, b.m_firstIndex, b.m_vertexOffset, b.m_firstInstance);
        }
        commands->EndRenderPass(commandList);
        commands->EndDebugRegion(commandList);
        return;
    }
    if (!surface || !radiance) return;
    if (!m_surfaceBindings) {
        m_surfaceBindings = driver->CreateShaderBindings();
        m_surfaceBindings->GetOrAddShaderBinding("surface")->m_buffer = surface;
        m_surfaceBindings->GetOrAddShaderBinding("radiance")->m_buffer = radiance;
    }
    std::string tag;
    commands->BeginDebugRegion(commandList, std::string(GetName()) + (TryGetString("Tag", tag) ? " QueueTag:" + tag : ""));
    // binding sets as RenderSceneNode.cpp:181-185: { frame, lights(+culled+grid+shadowMaps+lightsMatrices), per-draw data }
    commands->Dispatch(commandList, m_pShader, 0, 0, 0, { sceneView.m_frameBindings, sceneView.m_rhiLightsData, m_surfaceBindings });
    commands->EndDebugRegion(commandList);
}

void RenderSceneNode::Clear()
{
    m_pShader.Clear();
    m_pMaterial.Clear();
    m_pCutoutShader.Clear();
    for (auto& v : m_pVariants) v.Clear();
    m_pGltfShader.Clear();
    m_pGltfCutoutShader.Clear();
    for (auto& v : m_pGltfMaterials) v.Clear();
    for (auto& v : m_pTransparentMaterials) v.Clear();
    m_surfaceBindings.Clear();
    m_draws.Clear();
}

// ---- SceneIndirectDraws: RHIRecordDrawCall / RHIRecordDrawCallGPUCulling (RHI/Batch.hpp:53-191, :193-290) -------------------------------------
RHIShaderBindingSetPtr SceneIndirectDraws::Update(RHICommandListPtr transferCommandList, const RHISceneViewSnapshot& sceneView, const TVector<size_t>& selected,
                                                  bool bGpuCulling, RHITexturePtr depthHighZ)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    m_numCommands = 0;
    auto sceneData = sceneView.m_sceneBindings ? sceneView.m_sceneBindings->Find("data") : RHIShaderBindingPtr();
    if (selected.empty() || !sceneData || !sceneData->m_buffer) return RHIShaderBindingSetPtr();
    // Batch.hpp:74-91: the indirect buffer grows with a slack, and is bound as "drawIndexedIndirect"
    const size_t indirectBufferSize = selected.size() * sizeof(SailorDrawIndexedIndirectData);
    if (!m_indirectBuffer || m_indirectBuffer->m_size < indirectBufferSize) {
        m_indirectBuffer = driver->CreateIndirectBuffer(indirectBufferSize + 256);
        if (!m_indirectBuffer) return RHIShaderBindingSetPtr();
        m_indirectBinding = driver->CreateShaderBindings();
        m_indirectBinding->GetOrAddShaderBinding("drawIndexedIndirect")->m_buffer = m_indirectBuffer;
    }
    // :137-160 the commands as the host writes them; under culling firstInstance addresses the node's own packed records
    TVector<SailorDrawIndexedIndirectData> drawIndirect;
    uint32_t totalNumInstances = 0;
    for (size_t i : selected) {
        const RHISceneBatch& b = sceneView.m_batches[i];
        SailorDrawIndexedIndirectData data {};
        data.indexCount = b.m_indexCount; data.instanceCount = b.m_instanceCount; data.firstIndex = b.m_firstIndex; data.vertexOffset = (int32_t)b.m_vertexOffset;
        data.firstInstance = bGpuCulling ? totalNumInstances : b.m_firstInstance;
        drawIndirect.push_back(data);
        totalNumInstances += b.m_instanceCount;
    }
    commands->BeginDebugRegion(transferCommandList, "Update Indirect Buffer");
    commands->UpdateBuffer(transferCommandList, m_indirectBuffer, drawIndirect.data(), indirectBufferSize, 0); // (:165)
    commands->EndDebugRegion(transferCommandList);
    m_numCommands = selected.size();
    if (!bGpuCulling) return sceneView.m_sceneBindings; // RHIRecordDrawCall: counts un-culled, no dispatch
    // the node's m_perInstanceData, refilled every frame (DepthPrepassNode.cpp:185-230): the compaction is in place and would otherwise corrupt the next
    // node's input.  The reference refills from the proxies' host arrays; the view's records are device-resident here, so the refill is a device copy.
    const size_t need = (size_t)(totalNumInstances ? totalNumInstances : 1u) * sizeof(SailorPerInstanceData);
    if (!m_instances || m_instances->m_size != need) {
        m_instances = driver->CreateBuffer(need);
        if (!m_instances) return RHIShaderBindingSetPtr();
        m_perInstanceData = driver->CreateShaderBindings();
        m_perInstanceData->GetOrAddShaderBinding("data")->m_buffer = m_instances;
    }
    // what the draws and the pass's resolve read: the node's compacted copy beside the view's tables of THIS frame (rebuilt every frame: the view's set may be
    // another one, with other tables, from one frame to the next)
    m_sceneBindings = driver->CreateShaderBindings();
    for (auto& kv : sceneView.m_sceneBindings->m_bindings) m_sceneBindings->m_bindings[kv.first] = kv.second;
    m_sceneBindings->m_bindings["data"] = m_perInstanceData->Find("data");
    uint32_t packed = 0;
    for (size_t i : selected) {
        const RHISceneBatch& b = sceneView.m_batches[i];
        commands->CopyBuffer(transferCommandList, sceneData->m_buffer, m_instances, (size_t)b.m_instanceCount * sizeof(SailorPerInstanceData),
                             (size_t)b.m_firstInstance * sizeof(SailorPerInstanceData), (size_t)packed * sizeof(SailorPerInstanceData));
        packed += b.m_instanceCount;
    }
    // RenderSceneNode.cpp:126-139 / DepthPrepassNode.cpp: the culling shader with OCCLUSION_CULLING and the "depthHighZ" attachment as a sampler, when resolved
    const bool occlusion = depthHighZ && depthHighZ->m_buffer;
    if (!m_pCullShader || occlusion != m_bCullOcclusion) {
        m_pCullShader = occlusion ? driver->CreateShader("Shaders/ComputeMeshCulling.shader", { "OCCLUSION_CULLING" }) : driver->CreateShader("Shaders/ComputeMeshCulling.shader");
        m_bCullOcclusion = occlusion;
    }
    m_cullBindings = driver->CreateShaderBindings();
    if (occlusion) driver->AddSamplerToShaderBindings(m_cullBindings, "depthHighZ", depthHighZ, 0);
    struct PushConstants { uint32_t m_numBatches = 0, m_numInstances = 0, m_firstInstanceIndex = 0; } constants; // (:174-184)
    constants.m_numBatches = (uint32_t)selected.size();
    constants.m_numInstances = totalNumInstances;
    constants.m_firstInstanceIndex = 0;
    if (totalNumInstances == 0) return m_sceneBindings;
    commands->BeginDebugRegion(transferCommandList, "GPU Culling");
    commands->Dispatch(transferCommandList, m_pCullShader, 256, 1, 1, { m_cullBindings, m_perInstanceData, m_indirectBinding, sceneView.m_frameBindings }, &constants,
                       sizeof constants); // (:188) the pyramid it reads is the previous frame's: the transfer list is submitted before the graphics list
    commands->EndDebugRegion(transferCommandList);
    return m_sceneBindings;
}

void SceneIndirectDraws::Draw(RHICommandListPtr commandList, const RHISceneBatch& batch, size_t i) const
{
    auto commands = Renderer::GetDriverCommands();
    commands->BindVertexBuffer(commandList, batch.m_vertexBuffer, 0);
    commands->BindIndexBuffer(commandList, batch.m_indexBuffer, 0);
    commands->DrawIndexedIndirect(commandList, m_indirectBuffer, i * sizeof(SailorDrawIndexedIndirectData), 1, sizeof(SailorDrawIndexedIndirectData)); // (:169)
}

void SceneIndirectDraws::Clear()
{
    m_indirectBuffer.Clear(); m_instances.Clear();
    m_indirectBinding.Clear(); m_perInstanceData.Clear(); m_sceneBindings.Clear(); m_cullBindings.Clear();
    m_pCullShader.Clear();
    m_numCommands = 0;
}

// ---- DepthPrepassNode (FrameGraph/DepthPrepassNode.cpp:50-303) ----------------------------------------------------------------------------------
const char* DepthPrepassNode::m_name = "DepthPrepass";

void DepthPrepassNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr transferCommandList, RHICommandListPtr commandList,
                               const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    auto resolved = [&](const char* name) -> RHITexturePtr { // GetRHIResource / GetResolvedAttachment: a per-frame target is looked up by its name
        if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
        auto it = m_unresolvedResourceParams.find(name);
        return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
    };
    auto depth = resolved("depthStencil");
    if (!depth || sceneView.m_batches.empty()) return;
    std::string tag, value;
    const bool tagged = TryGetString("Tag", tag);
    const bool clearDepth = TryGetString("ClearDepth", value) && value == "true";
    const bool gpuCulling = TryGetString("GPUCulling", value) && value == "true";
    TVector<size_t> selected;
    for (size_t i = 0; i < sceneView.m_batches.size(); i++)
        if (sceneView.m_batches[i].m_tag.empty() || (tagged && sceneView.m_batches[i].m_tag == tag)) selected.push_back(i);
    RHIShaderBindingSetPtr sceneSet = m_draws.Update(transferCommandList, sceneView, selected, gpuCulling, resolved("depthHighZ"));
    if (!sceneSet) return; // nothing of this queue in the view
    if (!m_pDepthShader) m_pDepthShader = driver->CreateShader("Shaders/DepthOnly.shader");
    commands->BeginDebugRegion(commandList, std::string(GetName()) + (tagged ? " QueueTag:" + tag : ""));
    commands->BeginRenderPass(commandList, TVector<RHITexturePtr> {}, depth, clearDepth); // no colour attachment
    RHIMaterialPtr bound;
    for (size_t k = 0; k < selected.size(); k++) {
        const RHISceneBatch& b = sceneView.m_batches[selected[k]];
        RHIMaterialPtr material;
        if (b.m_bAlphaCutout) { // IsRequiredCustomDepthShader(): the batch's material is its own depth material (:86-90, :107-115, :246-255)
            RHIShaderPtr& shader = m_pCutoutShaders[b.m_bGltf ? 1 : 0];
            if (!shader) shader = driver->CreateShader(b.m_bGltf ? "Shaders/Standard_glTF.shader" : "Shaders/Standard.shader", { "ALPHA_CUTOUT" });
            RHIMaterialPtr& variant = m_pCutoutMaterials[(b.m_bGltf ? 2 : 0) + (b.m_bDoubleSided ? 1 : 0)];
            if (!variant) { variant = driver->CreateMaterial(shader); variant->m_bDoubleSided = b.m_bDoubleSided; }
            material = variant;
        } else {
            RHIMaterialPtr& variant = m_pDepthMaterials[b.m_bDoubleSided ? 1 : 0];
            if (!variant) { variant = driver->CreateMaterial(m_pDepthShader); variant->m_bDoubleSided = b.m_bDoubleSided; }
            material = variant;
        }
        if (material.GetRawPtr() != bound.GetRawPtr()) {
            commands->BindMaterial(commandList, material);
            if (b.m_bAlphaCutout) commands->BindShaderBindings(commandList, material, { sceneView.m_frameBindings, sceneView.m_rhiLightsData, sceneSet });
            else commands->BindShaderBindings(commandList, material, { sceneView.m_frameBindings, sceneSet }); // DepthOnly.shader: frame and PerInstanceDataSSBO
            bound = material;
        }
        m_draws.Draw(commandList, b, k);
    }
    commands->EndRenderPass(commandList);
    commands->EndDebugRegion(commandList);
}

void DepthPrepassNode::Clear()
{
    m_pDepthShader.Clear();
    for (auto& s : m_pCutoutShaders) s.Clear();
    for (auto& m : m_pDepthMaterials) m.Clear();
    for (auto& m : m_pCutoutMaterials) m.Clear();
    m_draws.Clear();
}

// ---- EyeAdaptationNode (FrameGraph/EyeAdaptationNode.cpp:19-230) ----------------------------------------------------------------
const char* EyeAdaptationNode::m_name = "EyeAdaptation";

void EyeAdaptationNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr transferCommandList, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName()); // (:28)

    // BaseFrameGraphNode::GetResolvedAttachment: the resource handed in, or the per-frame target of that name
    auto resolved = [&](const char* name) -> RHITexturePtr {
        if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
        auto it = m_unresolvedResourceParams.find(name);
        return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
    };
    RHITexturePtr target = resolved("color"); // (:30)

    if (!m_pComputeHistogramShader) m_pComputeHistogramShader = driver->CreateShader("Shaders/ComputeHistogram.shader");      // (:32-38)
    if (!m_pComputeAverageShader) m_pComputeAverageShader = driver->CreateShader("Shaders/ComputeAverageLuminance.shader");   // (:40-46)
    if (!m_pToneMappingShader) { // (:48-60)
        std::string shaderPath, definesStr;
        if (!TryGetString("toneMappingShader", shaderPath) || shaderPath.empty()) { commands->EndDebugRegion(commandList); return; } // check(!shaderPath.empty())
        TryGetString("toneMappingDefines", definesStr);
        TVector<std::string> defines; // Utils::SplitString(definesStr, " ")
        std::istringstream words(definesStr);
        for (std::string d; words >> d;) defines.push_back(d);
        m_pToneMappingShader = driver->CreateShader(shaderPath, defines);
    }

    RHITexturePtr quarterResolution = resolved("hdrColor");  // (:62)
    RHITexturePtr fullResolution = resolved("colorSampler"); // (:63)
    if (!quarterResolution || !fullResolution) { commands->EndDebugRegion(commandList); return; } // check(quarterResolution) (:70)

    if (!m_computeHistogramShaderBindings) { // (:65-80)
        m_computeHistogramShaderBindings = driver->CreateShaderBindings();
        auto histogramRes = driver->AddSsboToShaderBindings(m_computeHistogramShaderBindings, "histogram", sizeof(uint32_t), HistogramShades, 0, true);
        driver->AddStorageImageToShaderBindings(m_computeHistogramShaderBindings, "s_texColor", quarterResolution, 1);
        static TVector<uint32_t> initialData(HistogramShades); // "We should init the buffer"
        commands->UpdateShaderBinding(transferCommandList, histogramRes, initialData.data(), sizeof(uint32_t) * HistogramShades, 0);
    }
    if (!m_averageLuminance) { // (:82-98)
        m_averageLuminance = driver->CreateRenderTarget({ 1, 1 }, 1, EFormat::R32_SFLOAT); // R16_SFLOAT there (:91): fp32 is its canonical form here
        commands->ImageMemoryBarrier(commandList, m_averageLuminance, EImageLayout::TransferDstOptimal);
        commands->ClearImage(commandList, m_averageLuminance, 0.5f, 0.5f, 0.5f, 0.5f);
    }
    if (!m_computeAverageShaderBindings) { // (:100-109)
        auto histogram = m_computeHistogramShaderBindings->GetOrAddShaderBinding("histogram");
        m_computeAverageShaderBindings = driver->CreateShaderBindings();
        driver->AddShaderBinding(m_computeAverageShaderBindings, histogram, "histogram", 0);
        driver->AddStorageImageToShaderBindings(m_computeAverageShaderBindings, "s_texColor", m_averageLuminance, 1);
    }
    if (!m_pToneMappingShader || !m_pComputeHistogramShader || !m_pComputeAverageShader || !target) { // (:111-117)
        commands->EndDebugRegion(commandList);
        return;
    }
    if (!m_postEffectMaterial) { // (:119-149)
        m_shaderBindings = driver->CreateShaderBindings();
        // (FillShadersLayout (:124) reflects the shader's sets; the driver knows Tonemapping.shader's one uniform block)
        const size_t uniformsSize = m_vectorParams.size() * sizeof(vec4); // "That should be enough to handle all the uniforms"
        if (uniformsSize > 0) driver->AddBufferToShaderBindings(m_shaderBindings, "data", uniformsSize, 0, EShaderBindingType::UniformBuffer);
        m_postEffectMaterial = driver->CreateMaterial(m_pToneMappingShader);
        for (const auto& v : m_vectorParams) { // SetMaterialParameter(cmd, bindings, "data.whitePoint", value) splits at the dot (RHI/GraphicsDriver.h:335-341)
            const size_t dot = v.first.find('.');
            if (dot == std::string::npos) continue;
            commands->SetMaterialParameter(transferCommandList, m_shaderBindings, v.first.substr(0, dot), v.first.substr(dot + 1), &v.second, sizeof(vec4));
        }
        auto wp = m_vectorParams.find("data.whitePoint");
        if (wp != m_vectorParams.end()) m_whitePointLum = (0.2125f * wp->second.x + 0.7154f * wp->second.y) + 0.0721f * wp->second.z; // (:142-145)
        driver->AddSamplerToShaderBindings(m_shaderBindings, "colorSampler", fullResolution, 1);                       // UpdateShaderBinding(bindings, name, texture) (:147)
        driver->AddSamplerToShaderBindings(m_shaderBindings, "averageLuminanceSampler", m_averageLuminance, 2);        // (:148)
    }
    {
        const float minLogLuminance = -8.0f, maxLogLuminance = 4.0f, eyeReaction = 3.6f; // (:154-156)
        const float logLuminanceRange = maxLogLuminance - minLogLuminance;
        float pushConstantsHistogramm[] = { minLogLuminance, 1.0f / logLuminanceRange };
        float timeCoeff = std::clamp(1.0f - std::exp2(-sceneView.m_deltaTime * eyeReaction), 0.0f, 1.0f);
        float pushConstantsAverage[] = { minLogLuminance, logLuminanceRange, (float)quarterResolution->GetExtent().x * quarterResolution->GetExtent().y, timeCoeff };

        commands->ImageMemoryBarrier(commandList, quarterResolution, EImageLayout::General); // ComputeRead (:172)
        commands->Dispatch(commandList, m_pComputeHistogramShader, (uint32_t)(quarterResolution->GetExtent().x / 16), (uint32_t)(quarterResolution->GetExtent().y / 16), 1,
                           { m_computeHistogramShaderBindings }, &pushConstantsHistogramm, sizeof(float) * 2); // (:173-176)
        commands->ImageMemoryBarrier(commandList, m_averageLuminance, EImageLayout::ComputeWrite);
        commands->Dispatch(commandList, m_pComputeAverageShader, 1, 1, 1, { m_computeAverageShaderBindings }, &pushConstantsAverage, sizeof(float) * 4); // (:179-182)
        commands->ImageMemoryBarrier(commandList, m_averageLuminance, EImageLayout::ShaderReadOnlyOptimal);
        commands->ImageMemoryBarrier(commandList, target, EImageLayout::ColorAttachmentOptimal);
    }
    commands->ImageMemoryBarrier(commandList, fullResolution, EImageLayout::ShaderReadOnlyOptimal); // (:187-188)

    commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { target }, RHITexturePtr());                       // (:192-200)
    commands->BindMaterial(commandList, m_postEffectMaterial);                                                         // (:205)
    commands->BindShaderBindings(commandList, m_postEffectMaterial, { sceneView.m_frameBindings, m_shaderBindings }); // (:215)
    commands->DrawIndexed(commandList, 6, 1, 0, 0, 0);                                                                 // (:217) the full-screen NDC quad
    commands->EndRenderPass(commandList);                                                                              // (:218)
    commands->EndDebugRegion(commandList);
}

void EyeAdaptationNode::Clear() // (:223-230)
{
    m_pToneMappingShader.Clear();
    m_postEffectMaterial.Clear();
    m_shaderBindings.Clear();
    m_pComputeHistogramShader.Clear();
    m_pComputeAverageShader.Clear();
}

// ---- PostProcessNode (FrameGraph/PostProcessNode.cpp:19-209) ---------------------------------------------------------------------
const char* PostProcessNode::m_name = "PostProcess";

void PostProcessNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr transferCommandList, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    // a per-frame target or a sampler published under that name (FrameGraphParser.cpp:190-195 resolves both kinds)
    auto byName = [&](const std::string& name) -> RHITexturePtr {
        if (auto t = frameGraph->GetRenderTarget(name)) return t;
        return frameGraph->GetSampler(name);
    };
    RHITexturePtr target = GetRHIResource("color").DynamicCast<RHITexture>(); // (:29-45; the MSAA surface has no counterpart here)
    if (!target) {
        auto it = m_unresolvedResourceParams.find("color");
        target = frameGraph->GetRenderTarget(it != m_unresolvedResourceParams.end() ? it->second : std::string("BackBuffer"));
    }
    if (!m_pShader) { // (:47-59)
        std::string shaderPath, definesStr;
        if (!TryGetString("shader", shaderPath) || shaderPath.empty()) return; // check(!shaderPath.empty())
        TryGetString("defines", definesStr);
        TVector<std::string> defines; // Utils::SplitString(definesStr, " "); `~` is YAML's null
        std::istringstream words(definesStr == "~" ? std::string() : definesStr);
        for (std::string d; words >> d;) defines.push_back(d);
        m_pShader = driver->CreateShader(shaderPath, defines);
    }
    if (!m_pShader || !m_pShader->IsReady() || !target) return; // (:61-64) a shader the backend has no entry point for records nothing

    std::string shaderPath;
    TryGetString("shader", shaderPath);
    commands->BeginDebugRegion(commandList, std::string(GetName()) + ":" + shaderPath); // (:66-67)
    if (!m_postEffectMaterial) { // (:69-108)
        m_shaderBindings = driver->CreateShaderBindings();
        driver->FillShadersLayout(m_shaderBindings, { m_pShader }, 1);                                                     // (:74)
        const size_t uniformsSize = std::max<size_t>(256, m_vectorParams.size() * sizeof(vec4));                           // (:77)
        driver->AddBufferToShaderBindings(m_shaderBindings, "data", uniformsSize, 0, EShaderBindingType::UniformBuffer); // (:78)
        m_postEffectMaterial = driver->CreateMaterial(m_pShader);                                                          // (:82)
        auto setParameter = [&](const std::string& name, const void* value, size_t size) { // SetMaterialParameter(cmd, bindings, "data.radius", value) splits at the dot
            const size_t dot = name.find('.');
            if (dot != std::string::npos) commands->SetMaterialParameter(transferCommandList, m_shaderBindings, name.substr(0, dot), name.substr(dot + 1), value, size);
        };
        for (const auto& v : m_vectorParams) setParameter(v.first, &v.second, sizeof(vec4)); // (:84-87)
        for (const auto& f : m_floatParams) setParameter(f.first, &f.second, sizeof(float)); // (:89-92)
        uint32_t slot = 1;
        for (const auto& r : m_resourceParams) { // (:94-107) every resource under its own name, `color` included
            if (auto texture = r.second.DynamicCast<RHITexture>()) driver->AddSamplerToShaderBindings(m_shaderBindings, r.first, texture, slot++);
        }
    }
    for (const auto& r : m_unresolvedResourceParams) { // (:110-125) per-frame targets and late samplers, looked up every frame
        if (r.first == "color") continue;
        if (auto texture = byName(r.second)) driver->AddSamplerToShaderBindings(m_shaderBindings, r.first, texture, 0);
        // (a name that resolves to nothing stays unbound: the draw is then refused with the invalid-argument status when it is submitted)
    }
    for (const auto& kv : m_shaderBindings->m_bindings) // (:138-149)
        if (kv.second->m_type == EShaderBindingType::CombinedImageSampler && !kv.second->m_textures.empty())
            commands->ImageMemoryBarrier(commandList, kv.second->m_textures[0], EImageLayout::ShaderReadOnlyOptimal);
    commands->ImageMemoryBarrier(commandList, target, EImageLayout::ColorAttachmentOptimal); // (:151)

    commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { target }, RHITexturePtr());                                                   // (:172-180)
    commands->BindMaterial(commandList, m_postEffectMaterial);                                                                                     // (:186)
    commands->BindShaderBindings(commandList, m_postEffectMaterial, { sceneView.m_frameBindings, m_shaderBindings, sceneView.m_rhiLightsData }); // (:189)
    commands->DrawIndexed(commandList, 6, 1, 0, 0, 0);                                                                                             // (:198) the full-screen NDC quad
    commands->EndRenderPass(commandList);                                                                                                          // (:199)
    commands->EndDebugRegion(commandList);
}

void PostProcessNode::Clear() // (:204-209)
{
    m_pShader.Clear();
    m_postEffectMaterial.Clear();
    m_shaderBindings.Clear();
}

// ---- BlitNode (FrameGraph/BlitNode.cpp:18-124, without the MSAA half) ---------------------------------------------------------------
const char* BlitNode::m_name = "Blit";

void BlitNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot&)
{
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName()); // (:27)
    RHITexturePtr src = GetRHIResource("src").DynamicCast<RHITexture>(), dst = GetRHIResource("dst").DynamicCast<RHITexture>(); // (:52-53)
    for (const auto& r : m_unresolvedResourceParams) { // (:55-65)
        if (r.first == "src") src = frameGraph->GetRenderTarget(r.second);
        else if (r.first == "dst") dst = frameGraph->GetRenderTarget(r.second);
    }
    if (src && dst) {
        const bool bIsDepthFormat = src->m_bDepthFormat || dst->m_bDepthFormat; // (:67)
        const ivec4 srcRegion { 0, 0, src->GetExtent().x, src->GetExtent().y }, dstRegion { 0, 0, dst->GetExtent().x, dst->GetExtent().y }; // (:82-83)
        commands->ImageMemoryBarrier(commandList, src, EImageLayout::TransferSrcOptimal); // (:85-86)
        commands->ImageMemoryBarrier(commandList, dst, EImageLayout::TransferDstOptimal);
        commands->BlitImage(commandList, src, dst, srcRegion, dstRegion, bIsDepthFormat ? ETextureFiltration::Nearest : ETextureFiltration::Linear); // (:88)
    }
    commands->EndDebugRegion(commandList); // (:123)
}

void BlitNode::Clear() {}

// ---- SkyNode (FrameGraph/SkyNode.cpp:209-834) -------------------------------------------------------------------------------------------
const char* SkyNode::m_name = "Sky";

void SkyNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr transferCommandList, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName()); // (:216)

    if (!m_pSkyShader) { // (:220-232) one asset, five permutations
        m_pSkyShader = driver->CreateShader("Shaders/Sky.shader", { "FILL" });
        m_pSkyEnvShader = driver->CreateShader("Shaders/Sky.shader", {});
        m_pSunShader = driver->CreateShader("Shaders/Sky.shader", { "SUN" });
        m_pComposeShader = driver->CreateShader("Shaders/Sky.shader", { "COMPOSE" });
        m_pCloudsShader = driver->CreateShader("Shaders/Sky.shader", { "CLOUDS" });
    }
    if (!m_pSunShaftsShader) m_pSunShaftsShader = driver->CreateShader("Shaders/SunShafts.shader"); // (:234-242)
    if (!m_pBlitShader) m_pBlitShader = driver->CreateShader("Shaders/Blit.shader");                // (:244-252)
    if (!m_pStarsShader) m_pStarsShader = driver->CreateShader("Shaders/Stars.shader");             // (:341-349)
    // (:254-339 the CloudsMap texture and the two noise volumes are not loaded or generated here: SetCloudTextures publishes them, or the node stays cloudless)

    if (!m_pSkyTexture) m_pSkyTexture = driver->CreateRenderTarget({ (int32_t)SkyResolution, (int32_t)SkyResolution }, 1, EFormat::R32G32B32A32_SFLOAT); // (:351-363)
    if (!m_pSunTexture) m_pSunTexture = driver->CreateRenderTarget({ (int32_t)SunResolution, (int32_t)SunResolution }, 1, EFormat::R32G32B32A32_SFLOAT); // (:365-377)
    if (!m_pCloudsTexture) { // (:379-393)
        const float size = std::min(frameGraph->GetViewport().x * CloudsResolutionFactor, frameGraph->GetViewport().y * CloudsResolutionFactor);
        m_pCloudsTexture = driver->CreateRenderTarget({ std::max((int32_t)size, 1), std::max((int32_t)size, 1) }, 1, EFormat::R32G32B32A32_SFLOAT);
    }
    // (:405-417) the reference waits for all eight shaders and the star mesh; the four permutations this backend always draws are what the node waits for
    // here, the clouds and the blit are looked at where they are drawn, the others stay "not ready" for good and their draws below are left out
    if (!m_pSkyShader->IsReady() || !m_pSkyEnvShader->IsReady() || !m_pSunShader->IsReady() || !m_pComposeShader->IsReady() || !m_pSkyTexture || !m_pSunTexture ||
        !m_pCloudsTexture) {
        commands->EndDebugRegion(commandList);
        return;
    }

    if (!m_pSkyMaterial) { // (:419-455)
        m_pShaderBindings = driver->CreateShaderBindings();
        driver->FillShadersLayout(m_pShaderBindings, { m_pSkyShader }, 1);
        const size_t uniformsSize = std::max(sizeof(SkyParams), m_vectorParams.size() * sizeof(vec4));
        driver->AddBufferToShaderBindings(m_pShaderBindings, "data", uniformsSize, 0, EShaderBindingType::UniformBuffer);
        driver->AddSamplerToShaderBindings(m_pShaderBindings, "skySampler", m_pSkyTexture, 1);
        driver->AddSamplerToShaderBindings(m_pShaderBindings, "sunSampler", m_pSunTexture, 2);
        driver->AddSamplerToShaderBindings(m_pShaderBindings, "cloudsSampler", m_pCloudsTexture, 6);
        if (auto linearDepth = GetRHIResource("linearDepth").DynamicCast<RHITexture>()) driver->AddSamplerToShaderBindings(m_pShaderBindings, "linearDepth", linearDepth, 9);
        m_pSkyMaterial = driver->CreateMaterial(m_pSkyShader);
        m_pSkyEnvMaterial = driver->CreateMaterial(m_pSkyEnvShader);
        m_pSunMaterial = driver->CreateMaterial(m_pSunShader);
        m_pComposeMaterial = driver->CreateMaterial(m_pComposeShader);
        m_pCloudsMaterial = driver->CreateMaterial(m_pCloudsShader);
        m_pSunShaftsMaterial = driver->CreateMaterial(m_pSunShaftsShader);
        m_pSunShaftsMaterial->m_blendMode = EBlendMode::Multiply; // renderStateMultiply (:453-454)
    }
    if (HasCloudTextures() && m_bCloudTexturesChanged) { // (:431-433) every time the caller publishes textures: the set must not keep the earlier, caller-owned ones
        driver->AddSamplerToShaderBindings(m_pShaderBindings, "cloudsMapSampler", m_pCloudsMapTexture, 3);
        driver->AddSamplerToShaderBindings(m_pShaderBindings, "cloudsNoiseLowSampler", m_pCloudsNoiseLowTexture, 4);
        driver->AddSamplerToShaderBindings(m_pShaderBindings, "cloudsNoiseHighSampler", m_pCloudsNoiseHighTexture, 5);
        m_bCloudTexturesChanged = false;
    }
    if (HasCloudTextures() && !m_pShaderBindings->Find("g_noiseSampler")) // (:439-440) looked for on every frame until the graph has it
        if (auto noise = frameGraph->GetSampler("g_noiseSampler")) driver->AddSamplerToShaderBindings(m_pShaderBindings, "g_noiseSampler", noise, 8);
    if (auto binding = m_pShaderBindings->Find("data")) // (:458-467) every frame
        commands->UpdateShaderBinding(transferCommandList, binding, &m_skyParams, sizeof(SkyParams));
    if (!m_pBlitCloudsMaterial) { // (:469-483)
        m_pBlitCloudsBindings = driver->CreateShaderBindings();
        driver->FillShadersLayout(m_pBlitCloudsBindings, { m_pBlitShader }, 1);
        driver->AddSamplerToShaderBindings(m_pBlitCloudsBindings, "colorSampler", m_pCloudsTexture, 0);
        m_pBlitCloudsMaterial = driver->CreateMaterial(m_pBlitShader);
        m_pBlitCloudsMaterial->m_blendMode = EBlendMode::AlphaBlending; // RenderState { .., EBlendMode::AlphaBlending, .. } (:476)
    }
    if (!m_pEnvCubemapBindings[0]) { // (:485-515) the six faces' frame data, with the camera position of the frame that creates them
        for (uint32_t face = 0; face < 6; face++) {
            m_pEnvCubemapBindings[face] = driver->CreateShaderBindings();
            driver->AddBufferToShaderBindings(m_pEnvCubemapBindings[face], "frameData", sizeof(UboFrameData), 0, EShaderBindingType::UniformBuffer);
            UboFrameData frameData {};
            sailor_host_sky_face_matrices((int32_t)face, frameData.view, frameData.projection, frameData.invProjection); // (:487-495, :504-507)
            for (int k = 0; k < 3; k++) frameData.cameraPosition[k] = sceneView.m_camera.m_world[12 + k];                // (:503)
            frameData.cameraPosition[3] = 1.0f;
            frameData.viewportSize[0] = 128; frameData.viewportSize[1] = 128;                                            // (:508)
            commands->UpdateShaderBinding(transferCommandList, m_pEnvCubemapBindings[face]->GetOrAddShaderBinding("frameData"), &frameData, sizeof(frameData));
        }
    }
    if (!m_pStarsMaterial) { // (:517-522)
        m_pStarsMaterial = driver->CreateMaterial(m_pStarsShader);
        m_pStarsMaterial->m_blendMode = EBlendMode::Additive; // RenderState { .., EBlendMode::Additive, EFillMode::Point, .. } (:520)
    }

    auto resolved = [&](const char* name) -> RHITexturePtr { // BaseFrameGraphNode::GetResolvedAttachment
        if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
        auto it = m_unresolvedResourceParams.find(name);
        return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
    };
    RHITexturePtr target = resolved("color"); // (:524)
    if (!target) { commands->EndDebugRegion(commandList); return; }

    auto fullScreenDraw = [&](const char* region, RHITexturePtr attachment, RHIMaterialPtr material, const TVector<RHIShaderBindingSetPtr>& sets) {
        commands->BeginDebugRegion(commandList, region);
        commands->ImageMemoryBarrier(commandList, attachment, EImageLayout::ColorAttachmentOptimal);
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { attachment }, RHITexturePtr());
        commands->BindMaterial(commandList, material);
        commands->BindShaderBindings(commandList, material, sets);
        commands->DrawIndexed(commandList, 6, 1, 0, 0, 0); // the full-screen NDC quad
        commands->EndRenderPass(commandList);
        commands->EndDebugRegion(commandList);
    };
    fullScreenDraw("Sky", m_pSkyTexture, m_pSkyMaterial, { sceneView.m_frameBindings, m_pShaderBindings }); // (:536-563)
    // (:565-603) without published cloud textures: the else branch, whatever the parameter says
    const bool bClouds = m_skyParams.cloudsDensity > 0.0f && m_pCloudsShader->IsReady() && HasCloudTextures();
    if (bClouds) {
        commands->PushConstants(commandList, m_pCloudsMaterial, sizeof(uint32_t), &m_ditherPatternIndex);
        fullScreenDraw("Clouds", m_pCloudsTexture, m_pCloudsMaterial, { sceneView.m_frameBindings, m_pShaderBindings });
    } else { // (:604-609)
        commands->ImageMemoryBarrier(commandList, m_pCloudsTexture, EImageLayout::TransferDstOptimal);
        commands->ClearImage(commandList, m_pCloudsTexture, 0.0f, 0.0f, 0.0f, 0.0f);
    }
    fullScreenDraw("Sun", m_pSunTexture, m_pSunMaterial, { sceneView.m_frameBindings, m_pShaderBindings });     // (:611-642)
    fullScreenDraw("Compose", target, m_pComposeMaterial, { sceneView.m_frameBindings, m_pShaderBindings });    // (:644-680)
    // (:682-747) "Stars & Clouds", three draws into the target: the star points, the clouds blit, the sun shafts.  The first and the last are recorded for a
    // driver that opted in to their shaders, the stars once the mesh has been published (the reference waits for its mesh task, :395-417).  The alpha-blended
    // clouds blit is drawn when the clouds were: over the cleared plane (alpha 0) the reference's blit leaves every colour and turns alpha a into 0 - a,
    // which for the target's alpha of +0 is +0 again -- leaving it out keeps the cloudless frame's record what it was
    if (m_pStarsShader->IsReady() && HasStars()) {
        commands->BeginDebugRegion(commandList, "Stars");
        commands->BindVertexBuffer(commandList, m_starsVertexBuffer, 0); // (:694-695)
        commands->BindIndexBuffer(commandList, m_starsIndexBuffer, 0);
        float model[16];                                                  // (:697-698) translate(mat4(1), cameraPosition) * m_starsModelView, SetLocation (:690) included
        sailor_host_sky_stars_model(&sceneView.m_camera.m_world[12], model);
        commands->ImageMemoryBarrier(commandList, target, EImageLayout::ColorAttachmentOptimal); // (:701)
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { target }, RHITexturePtr());  // (:704-712; no depth test: the depth attachment is not needed)
        commands->BindMaterial(commandList, m_pStarsMaterial);                                        // (:714-716)
        commands->BindShaderBindings(commandList, m_pStarsMaterial, { sceneView.m_frameBindings, m_pShaderBindings });
        commands->PushConstants(commandList, m_pStarsMaterial, sizeof(model), model);
        commands->DrawIndexed(commandList, m_starsCount, 1u, 0u, 0u, 0u);                             // (:720)
        commands->EndRenderPass(commandList);
        commands->EndDebugRegion(commandList);
    }
    if (bClouds && m_pBlitShader->IsReady()) fullScreenDraw("Blit Clouds", target, m_pBlitCloudsMaterial, { sceneView.m_frameBindings, m_pBlitCloudsBindings });
    if (m_pSunShaftsShader->IsReady()) fullScreenDraw("Sun Shafts", target, m_pSunShaftsMaterial, { sceneView.m_frameBindings, m_pShaderBindings });

    if (m_bIsDirty) { // (:749-818)
        RHICubemapPtr cubemap = frameGraph->GetSampler("g_skyCubemap");
        if (cubemap && !cubemap->m_bCubemap) cubemap.Clear(); // DynamicCast<RHICubemap>
        if (!cubemap) { // (:753-762)
            cubemap = driver->CreateCubemap({ (int32_t)EnvCubemapSize, (int32_t)EnvCubemapSize }, 8, EFormat::R32G32B32A32_SFLOAT);
            if (cubemap) {
                commands->ImageMemoryBarrier(commandList, cubemap, EImageLayout::ShaderReadOnlyOptimal);
                frameGraph->SetSampler("g_skyCubemap", cubemap);
            }
        }
        if (cubemap) { // (:764-805)
            const uint32_t face = m_updateEnvCubemapPattern;
            if (face < 6)
                fullScreenDraw("Generate Environment Map", cubemap->GetFace(face, 0), m_pSkyEnvMaterial, { m_pEnvCubemapBindings[face], m_pShaderBindings });
            else { // 6 and 7 both (:798-802)
                commands->ImageMemoryBarrier(commandList, cubemap, EImageLayout::TransferDstOptimal);
                commands->GenerateMipMaps(commandList, cubemap);
            }
        }
        if (m_updateEnvCubemapPattern == 7) { // (:807-816)
            m_bIsDirty = false;
            if (auto node = frameGraph->GetGraphNode("Environment").DynamicCast<EnvironmentNode>()) node->MarkDirty();
        }
        m_updateEnvCubemapPattern++;
    }
    commands->EndDebugRegion(commandList); // (:820)
    m_ditherPatternIndex++;                // (:822)
}

void SkyNode::Clear() // (:825-834)
{
    m_pSkyTexture.Clear(); m_pSunTexture.Clear();
    m_pSkyShader.Clear(); m_pSkyEnvShader.Clear();
    m_pSkyMaterial.Clear(); m_pSkyEnvMaterial.Clear();
    m_pShaderBindings.Clear();
}

// ---- DebugDrawNode (FrameGraph/DebugDrawNode.cpp:19-83) -----------------------------------------------------------------------------------
const char* DebugDrawNode::m_name = "DebugDraw";

void DebugDrawNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName()); // (:24)
    auto resolved = [&](const char* name) -> RHITexturePtr { // GetRHIResource / GetResolvedAttachment
        if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
        auto it = m_unresolvedResourceParams.find(name);
        return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
    };
    RHITexturePtr target = resolved("color"), depthAttachment = resolved("depthStencil");
    if (!depthAttachment) depthAttachment = frameGraph->GetRenderTarget("DepthBuffer"); // (:30-34)
    if (!target) return;                                                                // (:36-39, without EndDebugRegion there too)
    commands->ImageMemoryBarrier(commandList, target, EImageLayout::ColorAttachmentOptimal); // (:43-44)
    if (depthAttachment) commands->ImageMemoryBarrier(commandList, depthAttachment, EImageLayout::General);
    if (sceneView.m_debugContext) {
        // what the world records into the secondary list: DrawDebugMesh(projection * view) of the view's camera -- the matrices FillFrameData uploads
        UboFrameData frame {};
        float viewProjection[16];
        sailor_host_fill_frame_data(sceneView.m_camera.m_world, sceneView.m_camera.m_fov, sceneView.m_camera.m_aspect, sceneView.m_camera.m_zNear, sceneView.m_camera.m_zFar,
                                    frameGraph->GetViewport().x, frameGraph->GetViewport().y, sceneView.m_currentTime, sceneView.m_deltaTime, &frame);
        sailor_host_mat4_mul(frame.projection, frame.view, viewProjection);
        // RenderSecondaryCommandBuffers(cmd, { list }, { color }, depth, area, offset, no clear) (:51-76)
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { target }, depthAttachment);
        sceneView.m_debugContext->DrawDebugMesh(commandList, viewProjection);
        commands->EndRenderPass(commandList);
    }
    commands->EndDebugRegion(commandList); // (:78)
}

void DebugDrawNode::Clear() {}

// ---- RenderImGuiNode (FrameGraph/RenderImGuiNode.cpp:21-60) over ImGuiApi::ImGui_RenderDrawData (Submodules/ImGuiApi.cpp:92-127, :190-276) --------------
const char* RenderImGuiNode::m_name = "RenderImGui";

void RenderImGuiNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName());
    auto resolved = [&](const char* name) -> RHITexturePtr { // GetRHIResource / GetResolvedAttachment
        if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
        auto it = m_unresolvedResourceParams.find(name);
        return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
    };
    RHITexturePtr target = resolved("color"), depthAttachment = frameGraph->GetRenderTarget("DepthBuffer"); // (:28-38)
    if (!target || !depthAttachment) return;                                                                // (:40-41, without EndDebugRegion there too)
    const RHIImGuiDrawData* ui = sceneView.m_drawImGui;
    if (!ui || !ui->m_material || !ui->m_vertexBuffer || !ui->m_indexBuffer) { // (no task: nothing was recorded, nothing to replay)
        commands->EndDebugRegion(commandList);
        return;
    }
    // ImGui_RenderDrawData (:197-275) through the flat form: the commands that are no callback and survive the clip test, with global offsets and scissors
    float pushConstants[4];
    uint32_t count = 0;
    int32_t width = 0, height = 0;
    TVector<SailorUiCommand> flat(ui->m_cmds.size() ? ui->m_cmds.size() : 1);
    const int st = sailor_host_ui_flatten(ui->m_displayPos, ui->m_displaySize, ui->m_framebufferScale, ui->m_lists.data(), (uint32_t)ui->m_lists.size(), ui->m_cmds.data(),
                                          (uint32_t)ui->m_cmds.size(), pushConstants, flat.data(), (uint32_t)flat.size(), &count, &width, &height);
    if (st == SAILOR_HIP_OK && width > 0 && height > 0) {
        commands->ImageMemoryBarrier(commandList, target, EImageLayout::ColorAttachmentOptimal);
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { target }, depthAttachment); // RenderSecondaryCommandBuffers(..., no clear) (:45-58)
        // ImGui_SetupRenderState (:92-127)
        commands->BindMaterial(commandList, ui->m_material);
        commands->BindVertexBuffer(commandList, ui->m_vertexBuffer, 0);
        commands->BindIndexBuffer(commandList, ui->m_indexBuffer, 0, true);
        commands->SetViewport(commandList, 0, 0, (float)width, (float)height, ivec2 { 0, 0 }, ivec2 { width, height }, 0, 1.0f);
        commands->PushConstants(commandList, ui->m_material, sizeof(pushConstants), pushConstants);
        for (uint32_t i = 0; i < count && i < flat.size(); i++) { // (:236-270)
            const SailorUiCommand& c = flat[i];
            commands->SetViewport(commandList, 0, 0, (float)width, (float)height, ivec2 { c.scissor[0], c.scissor[1] }, ivec2 { c.scissor[2], c.scissor[3] }, 0, 1.0f);
            commands->BindShaderBindings(commandList, ui->m_material, { ui->m_shaderBindings });
            commands->DrawIndexed(commandList, c.indexCount, 1, c.firstIndex, (uint32_t)c.vertexOffset, 0);
        }
        commands->EndRenderPass(commandList);
    }
    commands->EndDebugRegion(commandList);
}

void RenderImGuiNode::Clear() {}

// ---- BloomNode (FrameGraph/BloomNode.cpp:17-148) -------------------------------------------------------------------------------------------
const char* BloomNode::m_name = "Bloom";

void BloomNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot&)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    commands->BeginDebugRegion(commandList, GetName()); // (:28)

    RHITexturePtr bloomRenderTarget = GetRHIResource("bloom").DynamicCast<RHITexture>(); // GetResolvedAttachment("bloom") (:30)
    if (!bloomRenderTarget) {
        auto it = m_unresolvedResourceParams.find("bloom");
        if (it != m_unresolvedResourceParams.end()) bloomRenderTarget = frameGraph->GetRenderTarget(it->second);
    }
    if (!bloomRenderTarget) { commands->EndDebugRegion(commandList); return; }
    const size_t numMipBindings = bloomRenderTarget->GetMipLevels() - 1; // (:32)

    if (!m_pComputeDownscaleShader) m_pComputeDownscaleShader = driver->CreateShader("Shaders/ComputeBloomDownscale.shader"); // (:34-40)
    if (!m_pComputeUpscaleShader) m_pComputeUpscaleShader = driver->CreateShader("Shaders/ComputeBloomUpscale.shader");       // (:42-48)
    if (!m_pComputeUpscaleShader || !m_pComputeDownscaleShader || !m_pComputeUpscaleShader->IsReady() || !m_pComputeDownscaleShader->IsReady()) { // (:50-54)
        commands->EndDebugRegion(commandList);
        return;
    }

    if (m_computeUpscaleBindings.empty()) { // (:56-72)
        RHITexturePtr lensDirtTexture = frameGraph->GetSampler("g_lensDirtSampler");
        m_computeUpscaleBindings.resize(bloomRenderTarget->GetMipLevels());
        for (uint32_t i = (uint32_t)bloomRenderTarget->GetMipLevels() - 1; i >= 1; --i) {
            auto readMipLevel = bloomRenderTarget->GetMipLevel(i), writeMipLevel = bloomRenderTarget->GetMipLevel(i - 1); // GetMipLayer
            m_computeUpscaleBindings[i] = driver->CreateShaderBindings();
            driver->AddSamplerToShaderBindings(m_computeUpscaleBindings[i], "u_dirt_texture", lensDirtTexture, 2);
            driver->AddStorageImageToShaderBindings(m_computeUpscaleBindings[i], "u_input_texture", readMipLevel, 0);
            driver->AddStorageImageToShaderBindings(m_computeUpscaleBindings[i], "u_output_image", writeMipLevel, 1);
        }
    }
    if (m_computeDownscaleBindings.empty()) { // (:74-87)
        m_computeDownscaleBindings.resize(numMipBindings);
        for (uint32_t i = 0; i < bloomRenderTarget->GetMipLevels() - 1; ++i) {
            auto readMipLevel = bloomRenderTarget->GetMipLevel(i), writeMipLevel = bloomRenderTarget->GetMipLevel(i + 1);
            m_computeDownscaleBindings[i] = driver->CreateShaderBindings();
            driver->AddStorageImageToShaderBindings(m_computeDownscaleBindings[i], "u_input_texture", readMipLevel, 0);
            driver->AddStorageImageToShaderBindings(m_computeDownscaleBindings[i], "u_output_image", writeMipLevel, 1);
        }
    }

    auto vec = [&](const char* name) { auto it = m_vectorParams.find(name); return it == m_vectorParams.end() ? vec4() : it->second; }; // GetVec4
    const vec4 threshold = vec("threshold"), knee = vec("knee"); // (:89-90)
    PushConstantsDownscale downscaleParams {};
    sailor_host_bloom_push_constants(threshold.x, knee.x, downscaleParams.m_threshold); // (:93)

    commands->ImageMemoryBarrier(commandList, bloomRenderTarget, EImageLayout::General); // (:95)
    for (uint32_t i = 0; i < bloomRenderTarget->GetMipLevels() - 1; ++i) { // Bloom Downscale (:98-116)
        downscaleParams.m_useThreshold = i == 0;
        auto readMipLevel = bloomRenderTarget->GetMipLevel(i), writeMipLevel = bloomRenderTarget->GetMipLevel(i + 1);
        const float mipSize[2] = { (float)writeMipLevel->GetExtent().x, (float)writeMipLevel->GetExtent().y };
        commands->ImageMemoryBarrier(commandList, readMipLevel, EImageLayout::General);       // ComputeRead
        commands->ImageMemoryBarrier(commandList, writeMipLevel, EImageLayout::ComputeWrite);
        commands->Dispatch(commandList, m_pComputeDownscaleShader, (uint32_t)std::ceil(mipSize[0] / 8), (uint32_t)std::ceil(mipSize[1] / 8), 1u,
                           { m_computeDownscaleBindings[i] }, &downscaleParams, sizeof(PushConstantsDownscale));
    }

    PushConstantsUpscale upscaleParams {}; // (:118-120)
    upscaleParams.m_bloomIntensity = vec("bloomIntensity").x;
    upscaleParams.m_dirtIntensity = vec("dirtIntensity").x;
    for (uint32_t i = (uint32_t)bloomRenderTarget->GetMipLevels() - 1; i >= 1; --i) { // Bloom Upscale (:123-141)
        auto readMipLevel = bloomRenderTarget->GetMipLevel(i), writeMipLevel = bloomRenderTarget->GetMipLevel(i - 1);
        const float mipSize[2] = { (float)writeMipLevel->GetExtent().x, (float)writeMipLevel->GetExtent().y };
        upscaleParams.m_mipLevel = i;
        commands->ImageMemoryBarrier(commandList, readMipLevel, EImageLayout::General);       // ComputeRead
        commands->ImageMemoryBarrier(commandList, writeMipLevel, EImageLayout::ComputeWrite);
        commands->Dispatch(commandList, m_pComputeUpscaleShader, (uint32_t)std::ceil(mipSize[0] / 8), (uint32_t)std::ceil(mipSize[1] / 8), 1u,
                           { m_computeUpscaleBindings[i] }, &upscaleParams, sizeof(PushConstantsUpscale));
    }
    commands->EndDebugRegion(commandList); // (:143)
}

void BloomNode::Clear() {} // (:146-148)

// ---- ClearNode (FrameGraph/ClearNode.cpp:19-109) ----------------------------------------------------------------------------------------------
const char* ClearNode::m_name = "Clear";

void ClearNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr, RHICommandListPtr commandList, const RHISceneViewSnapshot&)
{
    auto commands = Renderer::GetDriverCommands();
    // (:28-56) an RHISurface target: surfaces -- an MSAA target with its resolved twin -- are not mirrored, a `bIsSurface` target is a plain texture here
    RHITexturePtr dst = GetRHIResource("target").DynamicCast<RHITexture>(); // (:57-60)
    bool bIsDepthFormat = dst && dst->m_bDepthFormat;
    if (!dst) { // (:61-90) by name from m_unresolvedResourceParams
        for (const auto& r : m_unresolvedResourceParams) {
            if (r.first == "target") {
                dst = frameGraph->GetRenderTarget(r.second);
                // (:69-85) "MSAA render targets are resolved inside the VulkanDriver": the clear of the internal MSAA depth target has no counterpart, the path
                // has no MSAA.  The per-frame "DepthBuffer" is the driver's depth buffer there, a depth format whatever texture the host wrapped for it here
                bIsDepthFormat = dst && (dst->m_bDepthFormat || r.second == "DepthBuffer");
                break;
            }
        }
    }
    if (!dst) return; // (the reference dereferences it: a `.renderer` file naming no target is its caller's error)
    commands->ImageMemoryBarrier(commandList, dst, EImageLayout::TransferDstOptimal); // (:92)
    if (bIsDepthFormat) { // (:93-101)
        const float clearDepth = GetFloat("clearDepth"), clearStencil = GetFloat("clearStencil");
        commands->BeginDebugRegion(commandList, GetName());
        commands->ClearDepthStencil(commandList, dst, clearDepth, (uint32_t)clearStencil);
        commands->EndDebugRegion(commandList);
    } else { // (:102-108) in the target's storage format: the fp32 channels of its canonical form (FrameGraphParser.cpp canonical_format); level 0 of a mip chain
        const vec4 clearColor = GetVec4("clearColor");
        commands->BeginDebugRegion(commandList, GetName());
        commands->ClearImage(commandList, dst, clearColor.x, clearColor.y, clearColor.z, clearColor.w);
        commands->EndDebugRegion(commandList);
    }
}

void ClearNode::Clear() {} // (:111-113)

// ---- ShadowPrepassNode (FrameGraph/ShadowPrepassNode.cpp:20-376) --------------------------------------------------------------------------------
const char* ShadowPrepassNode::m_name = "ShadowPrepass";

RHIMaterialPtr ShadowPrepassNode::GetOrAddShadowMaterial(EShadowType shadowType) // (:20-45)
{
    auto& material = shadowType == EShadowType::EVSM ? m_shadowMaterial_Evsm : m_shadowMaterial_Pcf;
    if (!material) {
        auto driver = Renderer::GetDriver();
        auto pShader = shadowType == EShadowType::EVSM ? driver->CreateShader("Shaders/ShadowCaster.shader", { "EVSM" }) : driver->CreateShader("Shaders/ShadowCaster.shader");
        if (pShader && pShader->IsReady()) material = driver->CreateMaterial(pShader); // RenderState: depth test and write, ECullMode::Back, GreaterOrEqual (:39)
    }
    return material;
}

void ShadowPrepassNode::Process(RHIFrameGraphPtr, RHICommandListPtr transferCommandList, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    if (!m_pBlurVerticalShader) { // (:54-77)
        m_pBlurVerticalShader = driver->CreateShader("Shaders/Blur.shader", { "VERTICAL", "EVSM" });
        m_pBlurVerticalMaterial = driver->CreateMaterial(m_pBlurVerticalShader);
        m_pBlurHorizontalShader = driver->CreateShader("Shaders/Blur.shader", { "HORIZONTAL", "EVSM" });
        m_pBlurHorizontalMaterial = driver->CreateMaterial(m_pBlurHorizontalShader);
        m_pBlurShaderBindings = driver->CreateShaderBindings();
        driver->FillShadersLayout(m_pBlurShaderBindings, { m_pBlurVerticalShader }, 1);
        RHIShaderBindingPtr blurDataBinding = driver->AddBufferToShaderBindings(m_pBlurShaderBindings, "data", sizeof(float) * 4 * 3, 0, EShaderBindingType::UniformBuffer);
        const float defaultBlurRadius = 3.0f;
        const float blurData[12] = { defaultBlurRadius, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
        commands->UpdateShaderBinding(transferCommandList, blurDataBinding, blurData, sizeof blurData);
    }
    // (:79 adds the binding again every frame, which finds it; here AddBufferToShaderBindings would zero a uniform block's bytes, so it is looked up)
    RHIShaderBindingPtr blurDataBinding = m_pBlurShaderBindings->Find("data");
    if (sceneView.m_shadowMapsToUpdate.empty()) return; // (:87-90)
    // (:81-85, behind the early return and every frame: the lights set's `lightsMatrices` may be replaced by a caller that hands maps in)
    m_lightMatrices = sceneView.m_rhiLightsData ? sceneView.m_rhiLightsData->Find("lightsMatrices") : RHIShaderBindingPtr();
    auto sceneData = sceneView.m_sceneBindings ? sceneView.m_sceneBindings->Find("data") : RHIShaderBindingPtr();
    if (!m_lightMatrices || !sceneData || !sceneData->m_buffer) return;

    commands->BeginDebugRegion(commandList, GetName()); // (:92)
    const uint32_t NumShadowPasses = (uint32_t)sceneView.m_shadowMapsToUpdate.size();
    // (:96-138) "Filter sceneView by tag": the passes arrive filtered -- m_bCastShadows is in their masks, the batches' runs are counted
    uint32_t numMeshes = 0;
    TVector<uint32_t> passFirst(NumShadowPasses);
    size_t words = 0;
    for (uint32_t passIndex = 0; passIndex < NumShadowPasses; passIndex++) {
        passFirst[passIndex] = numMeshes;
        numMeshes += sceneView.m_shadowMapsToUpdate[passIndex].m_numCasters;
        words = std::max(words, sceneView.m_shadowMapsToUpdate[passIndex].m_casterMask.size());
    }
    if (numMeshes == 0) { // (:140-143; the reference returns with the region open)
        commands->EndDebugRegion(commandList);
        return;
    }
    if (!m_perInstanceData || m_sizePerInstanceData < sizeof(PerInstanceData) * numMeshes) { // (:145-151) one SSBO for all passes
        m_perInstanceData = driver->CreateShaderBindings();
        driver->AddSsboToShaderBindings(m_perInstanceData, "data", sizeof(PerInstanceData), numMeshes, 0);
        m_sizePerInstanceData = sizeof(PerInstanceData) * numMeshes;
    }
    RHIShaderBindingPtr storageBinding = m_perInstanceData->GetOrAddShaderBinding("data"); // (:153)
    // (:155-201) the SSBO's contents: where the reference memcpys every batch's matrices on the host and uploads them, the passes' masks go to the device and the
    // runs are gathered there, in ascending instance order inside a run (the reference's order is its octree's walk; the rasteriser's result does not depend on it)
    const uint32_t numInstances = (uint32_t)(sceneData->m_buffer->m_size / sizeof(SailorPerInstanceData));
    const size_t maskBytes = words * 8;
    if (!m_masks || m_masks->m_size < NumShadowPasses * maskBytes) m_masks = driver->CreateBuffer(std::max<size_t>(NumShadowPasses, 4) * maskBytes);
    if (!m_masks || !storageBinding->m_buffer) { commands->EndDebugRegion(commandList); return; }
    TVector<IGraphicsDriverCommands::ShadowGatherRun> runs;
    for (uint32_t i = 0; i < NumShadowPasses; i++) {
        const auto& shadowPass = sceneView.m_shadowMapsToUpdate[i];
        if (shadowPass.m_numCasters == 0) continue;
        commands->UpdateBuffer(transferCommandList, m_masks, shadowPass.m_casterMask.data(), shadowPass.m_casterMask.size() * 8, i * maskBytes);
        for (size_t b = 0; b < shadowPass.m_batchRuns.size() && b < sceneView.m_batches.size(); b++) {
            const RHISceneBatch& batch = sceneView.m_batches[b];
            if (shadowPass.m_batchRuns[b].m_count == 0) continue;
            IGraphicsDriverCommands::ShadowGatherRun run;
            run.m_maskOffset = i * maskBytes;
            run.m_begin = std::min(batch.m_firstInstance, numInstances);
            run.m_end = (uint32_t)std::min<uint64_t>((uint64_t)batch.m_firstInstance + batch.m_instanceCount, std::min<uint64_t>(numInstances, shadowPass.m_casterMask.size() * 64));
            run.m_dstFirst = passFirst[i] + shadowPass.m_batchRuns[b].m_offset; // storageIndex[j] (:182)
            run.m_capacity = shadowPass.m_batchRuns[b].m_count;
            runs.push_back(run);
        }
    }
    commands->GatherShadowInstances(transferCommandList, sceneData->m_buffer, numInstances, m_masks, storageBinding->m_buffer, runs); // (in place of :194-201)
    // the caster draws' vertex input
    TVector<std::pair<RHIBufferPtr, RHIBufferPtr>> positions;
    auto positionsOf = [&](const RHIBufferPtr& vertexBuffer) -> RHIBufferPtr {
        if (!vertexBuffer) return RHIBufferPtr();
        for (auto& p : positions) if (p.first.GetRawPtr() == vertexBuffer.GetRawPtr()) return p.second;
        for (auto& p : m_positions) if (p.first.GetRawPtr() == vertexBuffer.GetRawPtr()) { positions.push_back(p); return p.second; }
        const uint32_t numVertices = (uint32_t)(vertexBuffer->m_size / sizeof(SailorVertexP3N3T3B3UV2C4));
        auto extracted = driver->CreateBuffer(std::max<size_t>((size_t)numVertices * 12, 4));
        if (extracted) commands->ExtractVertexPositions(transferCommandList, vertexBuffer, numVertices, extracted);
        positions.emplace_back(vertexBuffer, extracted);
        return extracted;
    };
    for (const auto& batch : sceneView.m_batches) positionsOf(batch.m_vertexBuffer);
    m_positions = positions;

    // RHIRecordDrawCall / RHIDrawCall (RHI/Batch.hpp) for the batches of pass `from`, drawn inside the current render pass.  Plain DrawIndexed per batch, not an
    // indirect buffer: the counts are the host's own popcounts, so an indirect command would carry nothing the host does not know, and ShadowCaster.shader under
    // DrawIndexedIndirect stays refused by the backend (HipGraphicsDriver.cpp DrawIndexedIndirect).
    auto drawBatches = [&](uint32_t from, RHIMaterialPtr material) -> uint32_t {
        const auto& pass = sceneView.m_shadowMapsToUpdate[from];
        uint32_t drawn = 0;
        for (size_t b = 0; b < pass.m_batchRuns.size() && b < sceneView.m_batches.size(); b++) {
            const RHISceneBatch& batch = sceneView.m_batches[b];
            auto vertexPositions = positionsOf(batch.m_vertexBuffer);
            if (pass.m_batchRuns[b].m_count == 0 || !vertexPositions || !batch.m_indexBuffer) continue;
            commands->BindMaterial(commandList, material);
            commands->BindShaderBindings(commandList, material, { sceneView.m_frameBindings, m_perInstanceData }); // shaderBindingsByMaterial (:208-212)
            commands->BindVertexBuffer(commandList, vertexPositions, 0);
            commands->BindIndexBuffer(commandList, batch.m_indexBuffer, 0);
            commands->DrawIndexed(commandList, batch.m_indexCount, pass.m_batchRuns[b].m_count, batch.m_firstIndex, batch.m_vertexOffset,
                                  passFirst[from] + pass.m_batchRuns[b].m_offset);
            drawn++;
        }
        return drawn;
    };

    for (uint32_t index = 0; index < NumShadowPasses; index++) { // (:219-365)
        const auto& shadowPass = sceneView.m_shadowMapsToUpdate[index];
        auto material = GetOrAddShadowMaterial(shadowPass.m_shadowType);
        if (!material || !shadowPass.m_shadowMap) continue; // (:118-125 bIsDepthMaterialReady)
        RHITexturePtr depthAttachment = driver->GetOrAddTemporaryRenderTarget(EFormat::R32_SFLOAT, shadowPass.m_shadowMap->GetExtent()); // (:227) the depth buffer's format
        if (!depthAttachment) continue;
        commands->BeginDebugRegion(commandList, "Record Shadow Map Pass " + std::to_string(index)); // (:221-229)
        commands->ImageMemoryBarrier(commandList, shadowPass.m_shadowMap, EImageLayout::ColorAttachmentOptimal); // (:233)
        commands->ImageMemoryBarrier(commandList, depthAttachment, EImageLayout::General);                        // (:234)
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { shadowPass.m_shadowMap }, depthAttachment, true); // (:236-245) clears colour to 0 and depth to 0
        commands->PushConstants(commandList, material, 64, shadowPass.m_lightMatrix); // (:249)
        uint32_t drawn = drawBatches(index, material);                                // (:251-257)
        for (uint32_t dependencyPass : shadowPass.m_internalCommandsList)             // (:259-271) into the same attachment, without a clear
            if (dependencyPass < NumShadowPasses) drawn += drawBatches(dependencyPass, material);
        commands->UpdateShaderBinding(transferCommandList, m_lightMatrices, shadowPass.m_lightMatrix, 64, 64 * (size_t)shadowPass.m_lighMatrixIndex); // (:273-276)
        commands->EndRenderPass(commandList); // (:278)
        // the backend clears with the pass's first draw and writes the map behind its last; a pass that drew nothing leaves the render pass's own clear
        if (drawn == 0) commands->ClearImage(commandList, shadowPass.m_shadowMap, 0.0f, 0.0f, 0.0f, 0.0f);
        // (:283) `m_blurRadius.length() > 0.1f` is glm's member length(), the component count 2: every EVSM pass is blurred
        if (shadowPass.m_shadowType == EShadowType::EVSM && blurDataBinding) {
            RHITexturePtr blurAttachment = driver->GetOrAddTemporaryRenderTarget(shadowPass.m_shadowMap->m_format, shadowPass.m_shadowMap->GetExtent()); // (:285)
            if (blurAttachment) {
                commands->UpdateShaderBinding(commandList, blurDataBinding, shadowPass.m_blurRadius, sizeof(float) * 2); // (:286)
                commands->BeginDebugRegion(commandList, "Blur Horizontal"); // (:289-324)
                driver->AddSamplerToShaderBindings(m_pBlurShaderBindings, "colorSampler", shadowPass.m_shadowMap, 1);
                commands->ImageMemoryBarrier(commandList, shadowPass.m_shadowMap, EImageLayout::ShaderReadOnlyOptimal);
                commands->ImageMemoryBarrier(commandList, blurAttachment, EImageLayout::ColorAttachmentOptimal);
                commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { blurAttachment }, RHITexturePtr());
                commands->BindMaterial(commandList, m_pBlurHorizontalMaterial);
                commands->BindShaderBindings(commandList, m_pBlurHorizontalMaterial, { sceneView.m_frameBindings, m_pBlurShaderBindings });
                commands->DrawIndexed(commandList, 6, 1, 0, 0, 0);
                commands->EndRenderPass(commandList);
                commands->ImageMemoryBarrier(commandList, shadowPass.m_shadowMap, EImageLayout::ColorAttachmentOptimal);
                commands->ImageMemoryBarrier(commandList, blurAttachment, EImageLayout::ShaderReadOnlyOptimal);
                commands->EndDebugRegion(commandList);
                commands->BeginDebugRegion(commandList, "Blur Vertical"); // (:327-355)
                driver->AddSamplerToShaderBindings(m_pBlurShaderBindings, "colorSampler", blurAttachment, 1);
                commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { shadowPass.m_shadowMap }, RHITexturePtr());
                commands->BindMaterial(commandList, m_pBlurVerticalMaterial);
                commands->BindShaderBindings(commandList, m_pBlurVerticalMaterial, { sceneView.m_frameBindings, m_pBlurShaderBindings });
                commands->DrawIndexed(commandList, 6, 1, 0, 0, 0);
                commands->EndRenderPass(commandList);
                commands->EndDebugRegion(commandList);
                driver->ReleaseTemporaryRenderTarget(blurAttachment); // (:357)
            }
        }
        driver->ReleaseTemporaryRenderTarget(depthAttachment); // (:360)
        commands->EndDebugRegion(commandList);
    }
    commands->EndDebugRegion(commandList); // (:367)
}

void ShadowPrepassNode::Clear() // (:370-376)
{
    m_lightMatrices.Clear();
    m_perInstanceData.Clear();
    m_shadowMaterial_Pcf.Clear();
    m_shadowMaterial_Evsm.Clear();
    m_masks.Clear();
    m_positions.clear();
}

// ---- ParticlesNode (FrameGraph/ParticlesNode.cpp:22-264) ------------------------------------------------------------------------------------------
const char* ParticlesNode::m_name = "ExperimentalParticles";

void ParticlesNode::SetParticles(const Header& header, std::vector<ParticleData> records, RHIBufferPtr vertexBuffer, RHIBufferPtr indexBuffer, uint32_t indexCount,
                                 uint32_t materialInstance)
{
    m_particlesHeader = header;
    m_particlesHeader.m_bIsLoaded = true; // (:48-51)
    m_particlesDataBinary = std::move(records);
    m_vertexBuffer = vertexBuffer; m_indexBuffer = indexBuffer; m_indexCount = indexCount; m_materialInstance = materialInstance;
    m_instances.Clear(); m_particlesFrames.Clear(); m_perInstanceData.Clear(); m_numInstances = 0; // (built again from the new records)
}

void ParticlesNode::Process(RHIFrameGraphPtr frameGraph, RHICommandListPtr transferCommandList, RHICommandListPtr commandList, const RHISceneViewSnapshot& sceneView)
{
    auto driver = Renderer::GetDriver();
    auto commands = Renderer::GetDriverCommands();
    std::string particlesPath;
    if (!m_particlesHeader.m_bIsLoaded || !TryGetString("particlesData", particlesPath)) return; // (:35-57) nothing loaded: silently
    if (!m_shadowMap) { // (:59-70) Linear, Clamp; 4096 x 4096 there
        m_shadowMap = driver->CreateRenderTarget(m_shadowMapExtent, 1, EFormat::R32_SFLOAT);
        m_shadowMapBinding = driver->CreateShaderBindings();
        driver->AddSamplerToShaderBindings(m_shadowMapBinding, "shadowMapSampler", m_shadowMap, 0);
    }
    if (!m_material || !m_shadowMaterial) { // (:72-105)
        std::string particleModel, particleShadowMaterial;
        if (!TryGetString("particleModel", particleModel)) return;
        if (!TryGetString("particleShadowMaterial", particleShadowMaterial)) return;
        if (!m_vertexBuffer || !m_indexBuffer || m_indexCount < 3) return; // m_mesh
        // Particle.mat / ParticleShadow.mat: Particle.shader without and with SHADOW_CASTER, cull Back, no blending; depth test and write for the first only
        m_material = driver->CreateMaterial(driver->CreateShader("Experimental/MeshParticles/Particle.shader"));
        m_shadowMaterial = driver->CreateMaterial(driver->CreateShader("Experimental/MeshParticles/Particle.shader", { "SHADOW_CASTER" }));
    }
    if (!m_pComputeShader) m_pComputeShader = driver->CreateShader("Experimental/MeshParticles/ComputeParticles.shader"); // (:107-113)
    if (!m_shadowMap || !m_material || !m_material->m_shader->IsReady() || !m_shadowMaterial || !m_shadowMaterial->m_shader->IsReady() || !m_pComputeShader->IsReady())
        return; // (:115-118)
    if (!m_instances) { // (:120-164) once, on the host
        const uint32_t count = m_particlesHeader.m_n * m_particlesHeader.m_traceFrames;
        if (count == 0 || m_particlesDataBinary.size() < m_particlesHeader.m_n) return;
        std::vector<PerInstanceData> instances(count);
        for (uint32_t i = 0; i < count; i++) {
            const ParticleData& p = m_particlesDataBinary[i / m_particlesHeader.m_traceFrames];
            PerInstanceData inst {};
            inst.model[0] = inst.model[5] = inst.model[10] = p.size2; // Transform { position (x2, y2, z2), scale size2 }.Matrix()
            inst.model[12] = p.xyz2[0]; inst.model[13] = p.xyz2[1]; inst.model[14] = p.xyz2[2]; inst.model[15] = 1.0f;
            inst.materialInstance = m_materialInstance;
            inst.color[0] = inst.color[1] = inst.color[2] = inst.color[3] = 1.0f;
            instances[i] = inst;
        }
        m_numInstances = count;
        m_perInstanceData = driver->CreateShaderBindings();
        auto data = driver->AddSsboToShaderBindings(m_perInstanceData, "data", sizeof(PerInstanceData), count, 0);
        auto frames = driver->AddSsboToShaderBindings(m_perInstanceData, "particlesData", sizeof(ParticleData), m_particlesDataBinary.size(), 1);
        m_instances = data ? data->m_buffer : RHIBufferPtr();
        m_particlesFrames = frames ? frames->m_buffer : RHIBufferPtr();
        if (!m_instances || !m_particlesFrames) { m_instances.Clear(); return; }
        // (CreateBuffer_Immediate there; here the uploads are recorded in front of the Dispatch on the same list)
        commands->UpdateBuffer(transferCommandList, m_instances, instances.data(), instances.size() * sizeof(PerInstanceData));
        commands->UpdateBuffer(transferCommandList, m_particlesFrames, m_particlesDataBinary.data(), m_particlesDataBinary.size() * sizeof(ParticleData));
        m_particlesDataBinary.clear(); // (:163)
    }
    auto resolved = [&](const char* name) -> RHITexturePtr {
        if (auto t = GetRHIResource(name).DynamicCast<RHITexture>()) return t;
        auto it = m_unresolvedResourceParams.find(name);
        return it == m_unresolvedResourceParams.end() ? RHITexturePtr() : frameGraph->GetRenderTarget(it->second);
    };
    RHITexturePtr colorAttachment = resolved("color"), depthAttachment = resolved("depthStencil"); // (:166-171)
    if (!depthAttachment) depthAttachment = frameGraph->GetRenderTarget("DepthBuffer");
    if (!colorAttachment || !depthAttachment) return;
    // (:173-175; the material's own set and the texture samplers hold nothing Particle.shader reads)
    TVector<RHIShaderBindingSetPtr> sets({ sceneView.m_frameBindings, sceneView.m_rhiLightsData, m_perInstanceData, m_shadowMapBinding });
    TVector<RHIShaderBindingSetPtr> computeSets({ m_perInstanceData, sceneView.m_frameBindings });
    PushConstants constants {}; // (:184-189)
    constants.numInstances = m_numInstances;
    constants.numFrames = m_particlesHeader.m_frames;
    constants.fps = m_particlesHeader.m_fps;
    constants.traceFrames = m_particlesHeader.m_traceFrames;
    constants.traceDecay = m_particlesHeader.m_traceDecay;
    commands->BeginDebugRegion(transferCommandList, GetName()); // (:191-193)
    commands->Dispatch(transferCommandList, m_pComputeShader, 256, 1, 1, computeSets, &constants, sizeof(constants));
    commands->EndDebugRegion(transferCommandList);

    commands->BeginDebugRegion(commandList, GetName()); // (:196) Shadows
    {
        commands->ImageMemoryBarrier(commandList, m_shadowMap, EImageLayout::ColorAttachmentOptimal);
        const ivec2 extent = m_shadowMap->GetExtent();
        commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { m_shadowMap }, RHITexturePtr(), true); // (:203-212) the only attachment, cleared to 0
        commands->BindMaterial(commandList, m_shadowMaterial);
        commands->SetViewport(commandList, 0.0f, (float)extent.y, (float)extent.x, -(float)extent.y, { 0, 0 }, extent, 0.0f, 1.0f); // (:215-220) flipped
        commands->BindShaderBindings(commandList, m_material, sets);
        commands->BindVertexBuffer(commandList, m_vertexBuffer, 0);
        commands->BindIndexBuffer(commandList, m_indexBuffer, 0);
        commands->DrawIndexed(commandList, m_indexCount, m_numInstances, 0, 0, 0);
        commands->EndRenderPass(commandList);
        commands->ImageMemoryBarrier(commandList, m_shadowMap, EImageLayout::ShaderReadOnlyOptimal);
    }
    commands->BeginRenderPass(commandList, TVector<RHITexturePtr> { colorAttachment }, depthAttachment, false); // (:232-240)
    const ivec2 extent = colorAttachment->GetExtent();
    commands->BindMaterial(commandList, m_material);
    commands->SetViewport(commandList, 0.0f, (float)extent.y, (float)extent.x, -(float)extent.y, { 0, 0 }, extent, 0.0f, 1.0f);
    commands->BindShaderBindings(commandList, m_material, sets);
    commands->BindVertexBuffer(commandList, m_vertexBuffer, 0);
    commands->BindIndexBuffer(commandList, m_indexBuffer, 0);
    commands->DrawIndexed(commandList, m_indexCount, m_numInstances, 0, 0, 0);
    commands->EndRenderPass(commandList);
    commands->EndDebugRegion(commandList); // (:259)
}

void ParticlesNode::Clear() {} // (:262-264)
