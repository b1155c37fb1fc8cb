// Mirrors Runtime/FrameGraph/ParticlesNode.{h,cpp} (Sailor::Framegraph::Experimental::ParticlesNode, "ExperimentalParticles"): per frame the Dispatch of
// ComputeParticles.shader on the transfer list, the node-owned R32_SFLOAT shadow map drawn with Particle.shader under SHADOW_CASTER, and the colour pass of
// Particle.shader into `color` / `depthStencil`.  Strings (ExperimentalRenderer.renderer:130-133): particlesData, particleModel, particleShadowMaterial.
// What the reference's loaders read (Particle_2.yaml's header, the .dat records, Particle.gltf's first mesh) is PUBLISHED here (SetParticles), as the Sky
// node's star catalogue is; without it Process returns early and silently, as the reference does while nothing is loaded (:54-57).
// In the reference this is a TFrameGraphNode<ParticlesNode>; here the class derives from the base directly and is created by
// FrameGraphBuilder::CreateOptInNode for graphs that enabled it, like BloomNode (FrameGraphNode.h says why).
#pragma once
#include <vector>
#include "FrameGraphNode.h"

namespace Sailor::Framegraph {

class ParticlesNode : public BaseFrameGraphNode {
public:
    struct Header { // ParticlesNode.h:22-42 (Particle_2.yaml)
        uint32_t m_n = 0, m_frames = 0, m_fps = 0, m_traceFrames = 0;
        float m_traceDecay = 0.0f;
        bool m_bIsLoaded = false;
    };
    using ParticleData = SailorParticleData;          // ParticlesNode.h:44-51
    using PushConstants = SailorParticlesConstants;   // :53-60
    using PerInstanceData = SailorParticleInstance;   // :62-71

    static const char* GetName() { return m_name; }
    std::string GetDebugName() const override { return m_name; }
    void Process(RHIFrameGraphPtr frameGraph, RHI::RHICommandListPtr transferCommandList, RHI::RHICommandListPtr commandList,
                 const RHI::RHISceneViewSnapshot& sceneView) override;
    void Clear() override;

    // what the loaders of ParticlesNode.cpp:35-52 and :89-101 would have loaded; the mesh buffers hold SailorVertexP3N3T3B3UV2C4 vertices and uint32 indices
    void SetParticles(const Header& header, std::vector<ParticleData> records, RHI::RHIBufferPtr vertexBuffer, RHI::RHIBufferPtr indexBuffer, uint32_t indexCount,
                      uint32_t materialInstance);
    void SetShadowMapExtent(RHI::ivec2 extent) { m_shadowMapExtent = extent; } // (:66 creates 4096 x 4096; before the first frame)
    RHI::RHITexturePtr GetShadowMap() const { return m_shadowMap; }
    RHI::RHIBufferPtr GetInstances() const { return m_instances; }

protected:
    static const char* m_name;
    Header m_particlesHeader;
    std::vector<ParticleData> m_particlesDataBinary;
    RHI::RHIBufferPtr m_vertexBuffer, m_indexBuffer; // m_mesh
    uint32_t m_indexCount = 0, m_materialInstance = 0;
    RHI::ivec2 m_shadowMapExtent { 4096, 4096 };
    RHI::RHITexturePtr m_shadowMap;
    RHI::RHIShaderBindingSetPtr m_shadowMapBinding, m_perInstanceData;
    RHI::RHIMaterialPtr m_material, m_shadowMaterial;
    RHI::RHIShaderPtr m_pComputeShader;
    RHI::RHIBufferPtr m_instances, m_particlesFrames;
    uint32_t m_numInstances = 0;
};

} // namespace Sailor::Framegraph
