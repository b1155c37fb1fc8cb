// The recording DepthPrepassNode.cpp and RenderSceneNode.cpp share, RHIRecordDrawCall / RHIRecordDrawCallGPUCulling (RHI/Batch.hpp:53-191, :193-290): every
// scene draw is a DrawIndexedIndirect over an indirect buffer the node owns and rewrites every frame; under `GPUCulling: true` the node also owns a
// per-instance SSBO it refills every frame, and a "GPU Culling" dispatch on the transfer list rewrites the commands' instanceCount and compacts those records
// before the graphics list's draws consume both.
#pragma once
#include "../RHI/Types.h"
#include "../RHI/SceneView.h"

namespace Sailor::Framegraph {

// What a node owns for its indirect draws (DepthPrepassNode.h: m_indirectBuffers, m_perInstanceData, m_cullingIndirectBufferBinding,
// m_computeMeshCullingBindings, m_pComputeMeshCullingShader; RenderSceneNode.h the same).
class SceneIndirectDraws {
public:
    // The frame's transfer work for the batches `selected` (indices into sceneView.m_batches, in drawing order):
    //   - the commands as the host writes them (Batch.hpp:148-153) into the indirect buffer ("Update Indirect Buffer");
    //   - bGpuCulling: the selected batches' instance records packed into the node's own SSBO in drawing order (firstInstance of a command = where its records
    //     start there, as storageIndex[j] + ssboOffset is), then the "GPU Culling" Dispatch with push constants { numBatches, numInstances,
    //     firstInstanceIndex } over { depthHighZ, data, drawIndexedIndirect, frame }; OCCLUSION_CULLING when `depthHighZ` is there.
    // Returns the scene set the draws bind: the view's own without culling, otherwise one whose `data` is the node's compacted copy (null: nothing to draw).
    RHI::RHIShaderBindingSetPtr Update(RHI::RHICommandListPtr transferCommandList, const RHI::RHISceneViewSnapshot& sceneView, const TVector<size_t>& selected,
                                       bool bGpuCulling, RHI::RHITexturePtr depthHighZ);
    // BindVertexBuffer / BindIndexBuffer / DrawIndexedIndirect of command i of the last Update
    void Draw(RHI::RHICommandListPtr commandList, const RHI::RHISceneBatch& batch, size_t i) const;
    void Clear();
    const RHI::RHIBufferPtr& GetIndirectBuffer() const { return m_indirectBuffer; }
    size_t GetNumCommands() const { return m_numCommands; }

private:
    RHI::RHIBufferPtr m_indirectBuffer, m_instances;
    size_t m_numCommands = 0;
    // m_sceneBindings is rebuilt every frame from the view's set of that frame (a small map): it never outlives the tables it names
    RHI::RHIShaderBindingSetPtr m_indirectBinding, m_perInstanceData, m_sceneBindings, m_cullBindings;
    RHI::RHIShaderPtr m_pCullShader;
    bool m_bCullOcclusion = false;
};

} // namespace Sailor::Framegraph
