// Mirrors the GPU-facing half of Runtime/ECS/LightingECS.{h,cpp}: the `light` SSBO (capacity LightsMaxNum records of
// LightShaderData, LightingECS.cpp:44), Tick's streaming of dirty runs (LightingECS.cpp:79-195: the skip list of static lights, inactive
// slots, dirtiness from the component or from its owner's transform, one UpdateShaderBinding per contiguous run) and FillLightingData
// (:373-406).  The owning game object is reduced to the two things Tick asks it: its mobility and the frame its transform last changed.
#pragma once
#include <vector>
#include "../RHI/GraphicsDriver.h"
#include "../RHI/SceneView.h"

namespace Sailor {

enum class ELightType : uint32_t { Directional = 0, Point = 1, Spot = 2, Area = 3 };          // Engine/Types.h:31-37
using EShadowType = RHI::EShadowType;                                                         // RHI/SceneView.h:13-18
enum class EMobilityType : uint8_t { Static = 0, Stationary = 1, Dynamic = 2 };               // Engine/Types.h:24-29

struct LightData { // ECS/LightingECS.h:18-33 (+ the owner transform's position / forward vector)
    float m_intensity[3] = { 100.0f, 100.0f, 100.0f };
    float m_attenuation[3] = { 1.0f, 0.022f, 0.0019f };
    float m_bounds[3] = { 100.0f, 100.0f, 100.0f };
    float m_cutOff[2] = { 30.0f, 45.0f }; // degrees
    ELightType m_type = ELightType::Point;
    EShadowType m_shadowType = EShadowType::PCF;
    float m_worldPosition[3] = { 0, 0, 0 };
    float m_direction[3] = { 0, 0, -1 };
    bool m_bIsDirty = true;                                   // ECS/ECS.h:38 (LightComponent marks a new light dirty)
    bool m_bIsActive = true;                                  // ECS/ECS.h:37
    size_t m_frameLastChange = 0;                             // ECS/ECS.h:36: the owner's frame this record was packed for
    size_t m_ownerFrameLastChange = 0;                        // GameObject::GetFrameLastChange(): the frame the owner's transform last changed
    EMobilityType m_ownerMobility = EMobilityType::Stationary; // Engine/GameObject.h:124
    // the owner's transform as PrepareCSMPasses needs it (RHILightProxy::m_lightTransform, :227-228): m_worldPosition above, and its rotation (x, y, z, w)
    float m_ownerRotation[4] = { 0.0f, 0.0f, 0.0f, 1.0f };
};

// What RHISceneView::TraceScene and the proxies give LightingECS::PrepareCSMPasses, flat over the scene's instances (`data` of the view's scene bindings):
// the world boxes on the device (what sailor_hip_ecs_sweep writes), m_bCastShadows as a bitmask (empty = every instance casts), the frame each instance last
// changed (RHISceneViewProxy::m_frame), how the overlap sets are traced, and the cascade maps' resolutions (ECS/LightingECS.h:67 unless overridden).
struct CsmCasterData {
    RHI::RHIBufferPtr m_worldAabb;
    uint32_t m_numInstances = 0;
    TVector<uint64_t> m_castShadows;
    TVector<uint64_t> m_lastChangedFrame;
    uint32_t m_traceMode = SAILOR_TRACE_FLAT_FLOAT_BOXES, m_rootSize = 0;
    RHI::ivec2 m_resolutions[SAILOR_NUM_CSM_CASCADES] = { { 4096, 4096 }, { 4096, 4096 }, { 4096, 4096 }, { 4096, 4096 } };
};

// One pass as the host half of PrepareCSMPasses decides it (:295-366), before it gets its map and matrix
struct CsmPassPlan {
    uint32_t m_cascade = 0;
    EShadowType m_shadowType = EShadowType::None;
    TVector<uint32_t> m_internalCommandsList;
    TVector<uint64_t> m_casterMask; // the final set, m_bCastShadows ANDed in
};

// One UpdateShaderBinding of LightingECS::Tick: `m_count` consecutive records written from record slot `m_startIndex` on.
struct LightUploadRun {
    size_t m_startIndex = 0;
    size_t m_count = 0;
};

class LightingECS {
public:
    static constexpr uint32_t LightsMaxNum = SAILOR_LIGHTS_MAX_NUM; // ECS/LightingECS.h:54
    using LightShaderData = SailorLightShaderData;                  // ECS/LightingECS.h:71-81

    explicit LightingECS(uint32_t capacity = LightsMaxNum);
    size_t RegisterComponent(const LightData& data);
    LightData& GetComponentData(size_t index) { return m_components[index]; }
    size_t Num() const { return m_components.size(); }
    // packs dirty lights and records one UpdateShaderBinding per contiguous dirty run into cmdList
    void Tick(RHI::RHICommandListPtr cmdList);
    // The loop of Tick without a driver (LightingECS.cpp:93-192): packs what is dirty, clears the flags, keeps the skip list of static lights up to
    // date and returns the runs in the order Tick issues them; `records` receives the runs' records back to back.
    static std::vector<LightUploadRun> CollectDirtyRuns(std::vector<LightData>& components, std::vector<std::pair<uint32_t, uint32_t>>& skipList,
                                                        std::vector<LightShaderData>& records);
    const std::vector<LightUploadRun>& GetLastUploads() const { return m_lastUploads; } // what the last Tick recorded
    // hands an already packed array over (synthetic frames): one upload
    void SetPacked(RHI::RHICommandListPtr cmdList, const LightShaderData* records, size_t count);
    void SetShadowMaps(const TVector<RHI::RHITexturePtr>& maps, const float* lightsMatrices64);
    void FillLightingData(RHI::RHISceneViewSnapshot& snapshot) const; // LightingECS.cpp:403-405
    RHI::RHIShaderBindingSetPtr GetLightsData() const { return m_lightsData; }

    // ---- the cascades (ECS/LightingECS.cpp:262-371, :373-406) ----
    static constexpr uint32_t NumCascades = SAILOR_NUM_CSM_CASCADES;   // ECS/LightingECS.h:65
    static constexpr uint32_t MaxShadowsInView = 1024;                  // ECS/LightingECS.h:53
    static constexpr float ShadowCascadeBlur[NumCascades][2] = { { 2, 5 }, { 1, 4 }, { 1, 3 }, { 1, 2 } }; // ECS/LightingECS.h:68
    ~LightingECS();
    // The scene's caster data (null = none: FillShadowPasses then leaves the snapshot's list empty and the bindings alone, as before this existed)
    void SetCasterData(const CsmCasterData* casters);
    bool HasCasterData() const { return m_bHasCasters; }
    // The host half of PrepareCSMPasses for ONE directional light (:283-367), on overlap sets that are already there: the cascades' shadow types (:303), the
    // removal, the snapshot comparison and the snapshots' update through sailor_host_csm_plan_passes, the dependency indices `alreadyPlacedPasses + shift`
    // (:307-331), m_bCastShadows (ShadowPrepassNode.cpp:110).  overlapMasks: NumCascades x ceil(numInstances / 64) words.  No device.
    static TVector<CsmPassPlan> PlanLightPasses(SailorCsmSnapshots* snapshots, uint32_t firstSnapshot, uint32_t alreadyPlacedPasses, uint32_t numInstances,
                                                const uint64_t* overlapMasks, EShadowType lightShadowType, const uint64_t* lastChangedFrame,
                                                const SailorCsmView* view, const uint64_t* castShadows);
    // per batch of the view: the popcount of the pass's mask over the batch's instance range, and the runs' offsets (in batch order)
    static uint32_t CountBatchRuns(const TVector<uint64_t>& mask, const TVector<RHI::RHISceneBatch>& batches, TVector<RHI::RHIShadowBatchRun>& outRuns);
    // FillLightingData's shadow half (:377-401) for the snapshot's one camera: GetLightsInFrustum, PrepareCSMPasses -> snapshot.m_shadowMapsToUpdate.  The
    // overlap sets come from sailor_hip_csm_caster_masks[_traced] over the caster data's boxes and cross to the host for the planning (one wait per frame).
    int FillShadowPasses(RHI::RHISceneViewSnapshot& snapshot);
    const TVector<RHI::RHITexturePtr>& GetCsmShadowMaps() const { return m_csmShadowMaps; }

private:
    int EnsureCsmShadowMaps(EShadowType firstCascadeType);
    bool m_bHasCasters = false;
    CsmCasterData m_casters;
    TVector<RHI::RHITexturePtr> m_csmShadowMaps;   // :53-63, owned here, persistent across frames
    EShadowType m_csmFirstCascadeType = EShadowType::None;
    RHI::RHIBufferPtr m_csmMasks;                  // NumCascades x words, device
    SailorCsmSnapshots* m_csmSnapshots = nullptr;  // LightingECS::m_csmSnapshots
    std::vector<LightData> m_components;
    std::vector<std::pair<uint32_t, uint32_t>> m_skipList; // (first slot, count) runs of static lights Tick steps over (LightingECS.h:106)
    std::vector<LightUploadRun> m_lastUploads;
    size_t m_packedCount = 0;
    RHI::RHIShaderBindingSetPtr m_lightsData;
};

// Flat form of TransformECS + StaticMeshRendererECS for the sweep (ECS/TransformECS.cpp:144-212, StaticMeshRendererECS.cpp:40-58)
class EcsSweepSystem {
public:
    EcsSweepSystem(const SailorTransform* transforms, const uint32_t* parent, const SailorAABB* localAabb, uint32_t count,
                   const uint32_t* levelOffsets, uint32_t numLevels);
    int Tick(const float* cameraWorld, float aspect, float fovDegrees, float zNear, float zFar);
    // How Tick decides visibility: SAILOR_TRACE_FLAT_FLOAT_BOXES (the default) tests the float world boxes; SAILOR_TRACE_OCTREE_INT_BOXES gives
    // RHISceneView::TraceScene's set as the reference computes it (integer boxes in the octree, RHI/SceneView.cpp:170) and fills m_inserted too.
    // rootSize 0 = SAILOR_OCTREE_ROOT_SIZE.
    void SetTraceMode(uint32_t mode, uint32_t rootSize = 0);
    uint32_t GetTraceMode() const { return m_traceMode; }
    uint32_t GetRootSize() const { return m_rootSize; }
    RHI::RHIBufferPtr m_transforms, m_parent, m_localAabb, m_world, m_worldAabb, m_visibility;
    RHI::RHIBufferPtr m_inserted; // octree mode: one bit per entity, in the octree at all
    uint32_t m_count = 0;
private:
    std::vector<uint32_t> m_levelOffsets;
    uint32_t m_traceMode = SAILOR_TRACE_FLAT_FLOAT_BOXES, m_rootSize = 0;
};

} // namespace Sailor
